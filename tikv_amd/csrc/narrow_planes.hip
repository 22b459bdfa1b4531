/* narrow_planes.hip — narrow companions of the decoded column planes and the
 * filter+count kernel over them. The wide planes, their build
 * and their consumers live in kernels.hip. */
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "copr_internal.h"
#include "fc_wait.h"                     /* FCW_* host word indices */

namespace copr {

/* ---------------- building a narrow plane ---------------------------------
 * A plane whose every row is PST_INT and whose values span less than 2^32
 * gets a companion holding (uint)(v - min) in 1, 2 or 4 bytes per row. The
 * filter+count kernel over it loads no state and a fraction of the value
 * bytes. */

/* one-time statistics over a wide plane: out[0] signed min, out[1] signed max
   over the PST_INT rows, out[2] the number of rows in any other state. The
   host seeds out with {INT64_MAX, INT64_MIN, 0}. */
__global__ void __launch_bounds__(256)
k_plane_stats(const int64_t *__restrict__ val, const uint8_t *__restrict__ st,
              uint64_t n_rows, long long *__restrict__ out) {
  long long mn = INT64_MAX, mx = INT64_MIN;
  unsigned long long other = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < n_rows; row += stride) {
    long long v = val[row];
    if (st[row] == PST_INT) {
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    } else {
      other++;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    long long omn = __shfl_down(mn, off, 64);
    long long omx = __shfl_down(mx, off, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    other += (unsigned long long)__shfl_down((long long)other, off, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMin(&out[0], mn);
    atomicMax(&out[1], mx);
    if (other) atomicAdd((unsigned long long *)&out[2], other);
  }
}

/* one-time narrowing pass: four rows per lane, two 16 B loads and one packed
   store. The last quad may read and write up to three rows past n_rows,
   inside both planes' tail slack. Widths 1 and 2; width 4 is k_plane_split. */
template <typename T>
struct alignas(4 * sizeof(T)) NarrowQuad { T r[4]; };

template <typename T>
__global__ void __launch_bounds__(256)
k_plane_narrow(const longlong2 *__restrict__ val, uint64_t n_rows,
               int64_t base, NarrowQuad<T> *__restrict__ out) {
  const uint64_t n_quads = (n_rows + 3) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       q < n_quads; q += stride) {
    longlong2 a = val[2 * q], b = val[2 * q + 1];
    NarrowQuad<T> o;
    o.r[0] = (T)((uint64_t)a.x - (uint64_t)base);
    o.r[1] = (T)((uint64_t)a.y - (uint64_t)base);
    o.r[2] = (T)((uint64_t)b.x - (uint64_t)base);
    o.r[3] = (T)((uint64_t)b.y - (uint64_t)base);
    out[q] = o;
  }
}

/* width 4: the same pass with the row split into two 16-bit
   planes, hi[row] = n >> 16 and lo[row] = n & 0xFFFF, one packed store each */
__global__ void __launch_bounds__(256)
k_plane_split(const longlong2 *__restrict__ val, uint64_t n_rows, int64_t base,
              NarrowQuad<uint16_t> *__restrict__ hi,
              NarrowQuad<uint16_t> *__restrict__ lo) {
  const uint64_t n_quads = (n_rows + 3) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       q < n_quads; q += stride) {
    longlong2 a = val[2 * q], b = val[2 * q + 1];
    const uint32_t n[4] = {(uint32_t)((uint64_t)a.x - (uint64_t)base),
                           (uint32_t)((uint64_t)a.y - (uint64_t)base),
                           (uint32_t)((uint64_t)b.x - (uint64_t)base),
                           (uint32_t)((uint64_t)b.y - (uint64_t)base)};
    NarrowQuad<uint16_t> h, l;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      h.r[j] = (uint16_t)(n[j] >> 16);
      l.r[j] = (uint16_t)n[j];
    }
    hi[q] = h;
    lo[q] = l;
  }
}

/* ---------------- a split plane's bucket index ----------------
 * off[h] = the first position of the sorted high halves holding a key >= h,
 * h = 0 .. 65536: one lane per h, a binary search each. */
__global__ void __launch_bounds__(256)
k_bucket_offsets(const uint16_t *__restrict__ keys, uint64_t n_rows,
                 unsigned long long *__restrict__ off) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h > COPR_N_BUCKETS) return;
  uint64_t lo = 0, hi = n_rows;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)keys[mid] < h) lo = mid + 1;
    else hi = mid;
  }
  off[h] = lo;
}

/* One stable radix sort of (H, L) pairs by H, the offsets from the sorted
   keys, one copy of them to the host. The sorted keys and the sort's
   temporary storage live for this call only. Whatever fails, the plane is as
   it was but for the verdict. */
static void bucket_index_build(DevRegion &rgn, DevRegion::ColPlane *p,
                               uint64_t budget_bytes, hipStream_t s,
                               uint64_t *built) {
  p->bkt_verdict = NAR_DECLINED;
  const uint64_t n = rgn.n_kv;
  const uint64_t off_bytes = (uint64_t)(COPR_N_BUCKETS + 1) * 8;
  const uint64_t cost = n * 2 + off_bytes;
  /* the sort has not been run here beyond 32-bit sizes */
  if (rgn.plane_bytes + cost > budget_bytes || n > 0xFFFFFFFFull) return;
  const uint16_t *hi = (const uint16_t *)p->nar;
  const uint16_t *lo = (const uint16_t *)((const uint8_t *)p->nar + p->nar_lo_off);
  uint16_t *d_keys = nullptr, *d_lo = nullptr;
  unsigned long long *d_off = nullptr;
  void *d_tmp = nullptr;
  uint64_t *h_off = (uint64_t *)malloc(off_bytes);
  size_t tmp_bytes = 0;
  bool ok = h_off != nullptr;
  ok = ok && rocprim::radix_sort_pairs(nullptr, tmp_bytes, hi, d_keys, lo, d_lo,
                                       (size_t)n, 0, 16, s) == hipSuccess;
  ok = ok && hipMalloc((void **)&d_keys, n * 2) == hipSuccess;
  ok = ok && hipMalloc((void **)&d_lo, n * 2 + 2048) == hipSuccess;
  ok = ok && hipMalloc((void **)&d_off, off_bytes) == hipSuccess;
  ok = ok && hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 1) == hipSuccess;
  ok = ok && rocprim::radix_sort_pairs(d_tmp, tmp_bytes, hi, d_keys, lo, d_lo,
                                       (size_t)n, 0, 16, s) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_bucket_offsets, dim3((COPR_N_BUCKETS + 1 + 255) / 256),
                       dim3(256), 0, s, d_keys, n, d_off);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(h_off, d_off, off_bytes, hipMemcpyDeviceToHost,
                            s) == hipSuccess;
  ok = ok && hipStreamSynchronize(s) == hipSuccess;
  /* what bucket_fc_fold relies on, checked once here */
  ok = ok && h_off[0] == 0 && h_off[COPR_N_BUCKETS] == n;
  for (uint32_t h = 0; ok && h < COPR_N_BUCKETS; h++)
    ok = h_off[h] <= h_off[h + 1];
  if (!ok) (void)hipGetLastError();
  hipFree(d_tmp);
  hipFree(d_keys);
  hipFree(d_off);
  if (!ok) {
    hipFree(d_lo);
    free(h_off);
    return;
  }
  p->bkt_lo = d_lo;
  p->bkt_off = h_off;
  p->bkt_verdict = NAR_BUILT;
  rgn.plane_bytes += cost;
  if (built) (*built)++;
}

static DevRegion::ColPlane *narrow_plane(DevRegion &rgn, int64_t col_id,
                                         uint64_t budget_bytes, hipStream_t s,
                                         uint64_t *built);

const DevRegion::ColPlane *dev_colplane_narrow(DevRegion &rgn, int64_t col_id,
                                               uint64_t budget_bytes,
                                               hipStream_t s, uint64_t *built,
                                               uint64_t bucket_min_rows,
                                               uint64_t *bkt_built) {
  DevRegion::ColPlane *p = narrow_plane(rgn, col_id, budget_bytes, s, built);
  if (p && p->nar_lo_off && p->bkt_verdict == NAR_UNTRIED &&
      rgn.n_kv >= bucket_min_rows)
    bucket_index_build(rgn, p, budget_bytes, s, bkt_built);
  return p;
}

static DevRegion::ColPlane *narrow_plane(DevRegion &rgn, int64_t col_id,
                                         uint64_t budget_bytes, hipStream_t s,
                                         uint64_t *built) {
  DevRegion::ColPlane *p = nullptr;
  for (int32_t i = 0; i < rgn.n_planes; i++)
    if (rgn.planes[i].col_id == col_id && rgn.planes[i].val)
      p = &rgn.planes[i];
  if (!p || !rgn.n_kv) return nullptr;
  if (p->nar_verdict == NAR_BUILT) return p;
  if (p->nar_verdict == NAR_DECLINED) return nullptr;
  /* whatever happens below is final: the passes never repeat */
  p->nar_verdict = NAR_DECLINED;
  long long h_st[3] = {INT64_MAX, INT64_MIN, 0};
  long long *d_st = nullptr;
  hipError_t e = hipMalloc((void **)&d_st, sizeof(h_st));
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_st, h_st, sizeof(h_st), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    uint32_t grid = (uint32_t)min((rgn.n_kv + 255) / 256, (uint64_t)4096);
    hipLaunchKernelGGL(k_plane_stats, dim3(grid), dim3(256), 0, s, p->val,
                       p->st, rgn.n_kv, d_st);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d_st);
  if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (h_st[2] != 0 || h_st[0] > h_st[1]) return nullptr;
  /* unsigned difference: a plane holding INT64_MIN and INT64_MAX gives
     2^64 - 1, not -1 */
  const uint64_t nmax = (uint64_t)h_st[1] - (uint64_t)h_st[0];
  const uint32_t w = nmax <= 0xFFull ? 1u : nmax <= 0xFFFFull ? 2u
                   : nmax <= 0xFFFFFFFFull ? 4u : 0u;
  if (!w) return nullptr;
  const uint64_t cost = rgn.n_kv * w;
  if (rgn.plane_bytes + cost > budget_bytes) return nullptr;
  /* a split plane is two planes of n_kv x 2 bytes, each with its own tail
     slack, the second on a 256 B boundary */
  const uint64_t lo_off =
      w == 4 ? (rgn.n_kv * 2 + 2048 + 255) & ~(uint64_t)255 : 0;
  void *nar = nullptr;
  if (hipMalloc(&nar, w == 4 ? lo_off + rgn.n_kv * 2 + 2048
                             : cost + 2048) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  const uint64_t n_quads = (rgn.n_kv + 3) >> 2;
  const uint32_t grid = (uint32_t)min((n_quads + 255) / 256, (uint64_t)4096);
  const longlong2 *src = (const longlong2 *)p->val;
  const int64_t base = (int64_t)h_st[0];
  switch (w) {
    case 1:
      hipLaunchKernelGGL(k_plane_narrow<uint8_t>, dim3(grid), dim3(256), 0, s,
                         src, rgn.n_kv, base, (NarrowQuad<uint8_t> *)nar);
      break;
    case 2:
      hipLaunchKernelGGL(k_plane_narrow<uint16_t>, dim3(grid), dim3(256), 0, s,
                         src, rgn.n_kv, base, (NarrowQuad<uint16_t> *)nar);
      break;
    default:
      hipLaunchKernelGGL(k_plane_split, dim3(grid), dim3(256), 0, s, src,
                         rgn.n_kv, base, (NarrowQuad<uint16_t> *)nar,
                         (NarrowQuad<uint16_t> *)((uint8_t *)nar + lo_off));
      break;
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    hipFree(nar);
    return nullptr;
  }
  p->nar = nar;
  p->nar_w = w;
  p->nar_lo_off = lo_off;
  p->nar_base = base;
  p->nar_nmax = nmax;
  p->nar_verdict = NAR_BUILT;
  rgn.plane_bytes += cost;
  if (built) (*built)++;
  return p;
}

/* The tail of the filter+count kernels below: every lane of a 256-lane block
 * brings the rows it kept.
 * The block's count goes to one of slot_mask + 1 count words, each on a
 * 128 B line of its own, chosen by block index: thousands of adds to one word
 * queue up at the end of the launch, spread over 64 they do
 * not.
 * With a ticket the launch finalizes the request: lane 0 of each block draws
 * a ticket once its add has returned, and the block that draws the last one
 * collects the count words, hands the host its three words and leaves count
 * words, ticket and stamp zero for the next request. Only atomics touch these
 * words, so no cache has to be written back or invalidated.
 * The request times itself. The launch that opens it has a
 * non-null stamp, the word COPR_FCN_STAMP_WORD behind the ticket, and its
 * block 0 reads the wall clock at entry (fcn_entry_clock) and stores it there
 * from this tail, so no wave waits for a round trip before its first loads.
 * When that launch also finalizes, the store is performed before block 0
 * draws its ticket, by the rule of the count add: an atomic with a return
 * value, waited for; relaxed atomics to two addresses are not ordered
 * otherwise. The finalizing block takes the stamp back, reads the clock again
 * and hands over (fcn_hand_over) to h_out, fine-grained pinned host memory
 * the host polls.
 * Solo: a launch with a stamp, a ticket and a grid of one block
 * opens the request, finalizes it and has nobody to order against, so its
 * block sum is the request's count and t_entry its stamp: no atomic, no
 * second barrier, straight to the hand-over. stamp && ticket is the right
 * condition: an earlier launch of the same request would have put its count
 * into the count words, and such a request's last launch has no stamp; the
 * words a solo launch leaves alone are zero when it starts and stay zero,
 * which is the state the ticket path leaves behind.
 * Assumption: block 0 starts no later than any other block's first load
 * matters. Workgroups are handed out in index order, so block 0 is in the
 * first wave of dispatches; the time between the dispatch packet and block
 * 0's first instruction is not in the figure (measured against the tracer's
 * durations in DESIGN §9n). */
__device__ __forceinline__ unsigned long long
fcn_entry_clock(const unsigned long long *stamp) {
  /* block-uniform, so the value lives in scalar registers through the loop */
  return (stamp && blockIdx.x == 0) ? wall_clock64() : 0ull;
}

/* The hand-over of a one-dispatch request to h_out, fine-grained
 * pinned host memory the host polls: FCW_COUNT and FCW_TICKS, a system-scope
 * fence, then seq in FCW_SEQ, which the host waits for, and a second fence.
 * A clock that did not advance reads as "no time", never as a wrapped
 * difference. seq is never 0 and new for every request. */
__device__ __forceinline__ void
fcn_hand_over(unsigned long long *__restrict__ h_out, unsigned long long tot,
              unsigned long long t0, unsigned long long t1,
              unsigned long long seq) {
  __hip_atomic_store(h_out + FCW_COUNT, tot, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(h_out + FCW_TICKS, t1 > t0 ? t1 - t0 : 0ull,
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __hip_atomic_store(h_out + FCW_SEQ, seq, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
}

__device__ __forceinline__ void
fcn_block_count(unsigned long long cnt, unsigned long long *__restrict__ cnt_out,
                uint32_t slot_mask, unsigned int *__restrict__ ticket,
                unsigned long long *__restrict__ h_out,
                unsigned long long *__restrict__ stamp,
                unsigned long long t_entry, unsigned long long seq) {
  __shared__ unsigned long long s_cnt[4];
  __shared__ unsigned int s_last;
  /* block-uniform, from kernel arguments and the grid alone */
  const bool solo = ticket && stamp && gridDim.x == 1;
  for (int off = 32; off > 0; off >>= 1)
    cnt += (unsigned long long)__shfl_down((long long)cnt, off, 64);
  if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (solo) {
    if (threadIdx.x == 0) {
      const unsigned long long tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      fcn_hand_over(h_out, tot, t_entry, wall_clock64(), seq);
    }
    return;
  }
  if (threadIdx.x == 0) {
    const unsigned long long b = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    unsigned long long *slot =
        cnt_out + (size_t)(blockIdx.x & slot_mask) * COPR_FCN_SLOT_STRIDE;
    unsigned int last = 0;
    /* the stamp and the add are in flight together; each has been performed
       once its old value is back, and one wait covers both. Without a ticket
       nobody waits: a later launch of the request is behind this one in the
       stream */
    unsigned long long old_s = 0, old_c = 0;
    if (stamp && blockIdx.x == 0)
      old_s = __hip_atomic_exchange(stamp, t_entry, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    if (!ticket) {
      if (b) atomicAdd(slot, b);
    } else {
      if (b)
        old_c = __hip_atomic_fetch_add(slot, b, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" :: "v"(old_s), "v"(old_c) : "memory");
      unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
      last = t == gridDim.x - 1 ? 1u : 0u;
    }
    s_last = last;
  }
  if (!ticket) return;
  __syncthreads();
  if (!s_last || threadIdx.x >= 64u) return;
  /* every block's add, and block 0's stamp, returned before its ticket was
     drawn, and this block drew the last ticket: the words are final */
  /* lane 0 takes the stamp back in the same breath as the lanes take the
     count words, so the two round trips overlap and the tail waits once */
  unsigned long long t0 = 0;
  if (threadIdx.x == 0)
    t0 = __hip_atomic_exchange(
        (unsigned long long *)ticket + COPR_FCN_STAMP_WORD, 0ull,
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long tot = 0;
  if (threadIdx.x <= slot_mask)
    tot = __hip_atomic_exchange(
        cnt_out + (size_t)threadIdx.x * COPR_FCN_SLOT_STRIDE, 0ull,
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int off = 32; off > 0; off >>= 1)
    tot += (unsigned long long)__shfl_down((long long)tot, off, 64);
  if (threadIdx.x == 0) {
    const unsigned long long t1 = wall_clock64();
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fcn_hand_over(h_out, tot, t0, t1, seq);
  }
}

/* The packed count of fold_packed_out (plane_fold.h, which mirrors this bit
 * for bit) over the eight 16-bit rows of one 16 B vector, two rows per
 * instruction and four instructions per word: subtract, subtract clamped at
 * zero, min with one, add. The counts stay packed, one per half of acc, and
 * packed_sum adds the halves; a half holds up to 0xFFFF, a lane's iteration
 * adds at most 16. Inline assembly: the compiler unpacks the clamped subtract
 * and the min when they are written with vector types. */
__device__ __forceinline__ uint32_t
packed_out_acc(uint4 v, uint32_t lo_pk, uint32_t span_pk, uint32_t acc) {
  const uint32_t ones = 0x00010001u;
  uint32_t t;
  /* one statement for the vector: the compiler pads every asm statement
     with an s_nop */
#define COPR_PK_OUT(W)                                                       \
  "v_pk_sub_u16 %0, " W ", %6\n\t"                                           \
  "v_pk_sub_u16 %0, %0, %7 clamp\n\t"                                        \
  "v_pk_min_u16 %0, %0, %8\n\t"                                              \
  "v_pk_add_u16 %1, %1, %0\n\t"
  asm(COPR_PK_OUT("%2") COPR_PK_OUT("%3") COPR_PK_OUT("%4") COPR_PK_OUT("%5")
      : "=&v"(t), "+v"(acc)
      : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "s"(lo_pk), "s"(span_pk),
        "s"(ones));
#undef COPR_PK_OUT
  return acc;
}
__device__ __forceinline__ uint32_t packed_sum(uint32_t acc) {
  return (acc & 0xFFFFu) + (acc >> 16);
}

/* Filter+count over a narrow plane of 1 or 2 bytes per row. Each lane loads
 * 16 B = 16 / sizeof(T) rows, UNR loads in flight, grid-stride; the row test
 * is the 32-bit form of k_plane_fc's (narrow_fc_fold, plane_fold.h). Every
 * row is a known int, so there is no state, no ABSENT fill and no parse
 * error. Loads are clamped to the last vector and rows masked by n_rows, as
 * in k_plane_fc; the last vector may read up to 15 B into the tail slack. */
template <typename T>
__global__ void __launch_bounds__(256)
k_plane_fcn(const uint4 *__restrict__ data, uint64_t n_rows, NarrowFcArgs nf,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  constexpr int UNR = 4;
  constexpr uint32_t R = 16u / sizeof(T);          /* rows per 16 B */
  constexpr uint32_t PW = 4u / sizeof(T);          /* rows per 32-bit word */
  const bool inv = nf.invert != 0;
  unsigned long long cnt = 0;
  const uint64_t n_vec = (n_rows + R - 1) / R;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  /* the packed count's constants; a 2-byte plane's lo + span <= 0xFFFF, and
     the "never" form's span saturates to every row */
  const uint32_t lo_pk = fold_pack16(nf.lo), span_pk = fold_pack16(nf.span);
  /* b0 = p0 - threadIdx.x, the block's first vector, kept beside p0 so that
     the compiler sees it is the same in every lane */
  uint64_t b0 = (uint64_t)blockIdx.x * 256u * UNR;
  for (uint64_t p0 = b0 + threadIdx.x; p0 < n_vec; p0 += step, b0 += step) {
    uint4 v[UNR];
    if constexpr (sizeof(T) == 2) {
      /* every row of the block's iteration is inside the plane (uniform):
         no clamp, no live mask, two rows per instruction */
      if ((b0 + 256u * UNR) * R <= n_rows) {
        #pragma unroll
        for (int u = 0; u < UNR; u++) v[u] = data[p0 + (uint64_t)u * 256u];
        __builtin_amdgcn_sched_barrier(0);
        uint32_t acc = 0;
        #pragma unroll
        for (int u = 0; u < UNR; u++)
          acc = packed_out_acc(v[u], lo_pk, span_pk, acc);
        const uint32_t out = packed_sum(acc);
        cnt += inv ? out : UNR * R - out;
        continue;
      }
    }
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
      v[u] = data[p];
    }
    /* all four loads issue before the first is used */
    __builtin_amdgcn_sched_barrier(0);
    uint32_t c = 0;
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      const uint64_t p = p0 + (uint64_t)u * 256u;
      /* rows of this vector inside the plane: R except in the last vector */
      uint32_t live = 0;
      if (p < n_vec) {
        const uint64_t left = n_rows - p * R;
        live = left < R ? (uint32_t)left : R;
      }
      const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      #pragma unroll
      for (uint32_t j = 0; j < R; j++) {
        uint32_t n = w[j / PW];
        if (sizeof(T) < 4)
          n = (n >> (8u * sizeof(T) * (j % PW))) & (uint32_t)(T)~(T)0;
        const bool keep = ((n - nf.lo) <= nf.span) != inv;
        c += (j < live && keep) ? 1u : 0u;
      }
    }
    cnt += c;
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

/* Filter+count over a split plane: k_plane_fcn's shape over the
 * high halves alone, 8 rows per 16 B load. Phase one counts the rows whose
 * high half decides them (split_row_in's "sure") and flags the live rows it
 * does not (maybe and not sure), one bit per row of the lane's four vectors.
 * Phase two, entered only by a wave that holds a flagged row, loads the low
 * halves of the flagged vectors (same index, same clamp), all of them before
 * the first is used, and puts the flagged rows through the full test. Rows at
 * or beyond n_rows are never flagged: the tail slack holds arbitrary bytes.
 * With every row flagged the low loads are as coalesced as the high ones and
 * the launch reads n_rows x 4 bytes, as k_plane_fcn<uint32_t> did.
 * An iteration whose every row is inside the plane first counts its rows
 * packed and classifies them one by one only in a wave that
 * holds an open row; the iteration with the plane's last vector classifies
 * every row under its live mask. */
__global__ void __launch_bounds__(256)
k_plane_fcs(const uint4 *__restrict__ hi, const uint4 *__restrict__ lo,
            uint64_t n_rows, SplitFcArgs sf,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  constexpr int UNR = 4;
  constexpr uint32_t R = 8;                        /* rows per 16 B */
  const bool inv = sf.invert != 0;
  unsigned long long cnt = 0;
  const uint64_t n_vec = (n_rows + R - 1) / R;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  /* b0 = p0 - threadIdx.x, the block's first vector, kept beside p0 so that
     the compiler sees it is the same in every lane */
  uint64_t b0 = (uint64_t)blockIdx.x * 256u * UNR;
  for (uint64_t p0 = b0 + threadIdx.x; p0 < n_vec; p0 += step, b0 += step) {
    uint4 v[UNR];
    /* one bit per row, vector u in bits 8u .. 8u + 7: the rows inside the
       plane and the open rows; in = the rows phase one decided in */
    uint32_t livem = ~0u, in = 0, amb = 0;
    bool classify = true;
    if ((b0 + 256u * UNR) * R <= n_rows) {
      /* Fast path: every row of the block's iteration is inside
         the plane, so there is no clamp and no live mask, and the rows are
         counted two per instruction, never unpacked: out_maybe and out_sure
         rows outside the two intervals. sure lies inside maybe, so the lane
         holds an open row exactly when the counts differ; only a wave with
         such a lane classifies its rows one by one, from the same registers. */
      #pragma unroll
      for (int u = 0; u < UNR; u++) v[u] = hi[p0 + (uint64_t)u * 256u];
      /* all four loads issue before the first is used */
      __builtin_amdgcn_sched_barrier(0);
      uint32_t acc_m = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++)
        acc_m = packed_out_acc(v[u], sf.maybe_lo_pk, sf.maybe_span_pk, acc_m);
      const uint32_t out_maybe = packed_sum(acc_m);
      /* an empty sure interval has no 16-bit form: every row is outside it */
      uint32_t out_sure = UNR * R;
      if (!sf.sure_empty) {
        uint32_t acc_s = 0;
        #pragma unroll
        for (int u = 0; u < UNR; u++)
          acc_s = packed_out_acc(v[u], sf.sure_lo_pk, sf.sure_span_pk, acc_s);
        out_sure = packed_sum(acc_s);
      }
      in = UNR * R - out_sure;
      classify = __builtin_amdgcn_ballot_w64(out_sure != out_maybe) != 0;
    } else {
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
        v[u] = hi[p];
      }
      /* all four loads issue before the first is used */
      __builtin_amdgcn_sched_barrier(0);
      livem = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        const uint64_t p = p0 + (uint64_t)u * 256u;
        uint32_t live = 0;
        if (p < n_vec) {
          const uint64_t left = n_rows - p * R;
          live = left < R ? (uint32_t)left : R;
        }
        livem |= ((1u << live) - 1u) << (u * R);
      }
    }
    if (classify) {             /* wave-uniform */
      uint32_t maybe = 0, sure = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        #pragma unroll
        for (uint32_t j = 0; j < R; j++) {
          const uint32_t h = (j & 1u) ? w[j / 2] >> 16 : w[j / 2] & 0xFFFFu;
          maybe |= (split_maybe(h, sf) ? 1u : 0u) << (u * R + j);
          sure |= (split_sure(h, sf) ? 1u : 0u) << (u * R + j);
        }
      }
      in = __popc(sure & livem);
      amb = maybe & ~sure & livem;
    }
    const unsigned long long open_lanes =
        __builtin_amdgcn_ballot_w64(amb != 0);
    if (open_lanes != 0) {
      uint4 lv[UNR];
      if (__popcll(open_lanes) >= 16) {
        /* dense (wave-uniform): a quarter of the wave holds an open row, so
           every lane loads its four vectors, unpredicated and coalesced */
        #pragma unroll
        for (int u = 0; u < UNR; u++)
          lv[u] = lo[min(p0 + (uint64_t)u * 256u, n_vec - 1)];
      } else {
        #pragma unroll
        for (int u = 0; u < UNR; u++) {
          lv[u] = make_uint4(0, 0, 0, 0);
          if ((amb >> (u * R)) & 0xFFu)
            lv[u] = lo[min(p0 + (uint64_t)u * 256u, n_vec - 1)];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      uint32_t full = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        const uint32_t wh[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        const uint32_t wl[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w};
        #pragma unroll
        for (uint32_t j = 0; j < R; j++) {
          const uint32_t h = (j & 1u) ? wh[j / 2] >> 16 : wh[j / 2] & 0xFFFFu;
          const uint32_t l = (j & 1u) ? wl[j / 2] >> 16 : wl[j / 2] & 0xFFFFu;
          full |= (split_full_in(h, l, sf) ? 1u : 0u) << (u * R + j);
        }
      }
      in += __popc(full & amb);
    }
    cnt += inv ? __popc(livem) - in : in;
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

/* Filter+count over a split plane's bucket index. The host has
 * counted the rows whose bucket decides them from two offsets (add, which
 * block 0 brings to the tail), so the kernel reads only the edge buckets' low
 * halves: up to two slices [beg, end) of bkt_lo, each with its h.
 * k_plane_fcn<uint16_t>'s shape over the concatenation of the two slices'
 * 16 B vectors: slice i covers the vectors vb[i] = beg / 8 up to
 * ceil(end / 8), vn[i] of them, a slice's first and last vector shared with
 * its neighbours in bkt_lo and masked by [beg, end). Loads are clamped to the
 * last vector of the concatenation, which may reach 14 B into the tail slack.
 * Within one bucket the full test is a 16-bit range test on l, so an iteration
 * whose every row is inside one slice is counted packed; the
 * others put each live row through split_full_in. A kept row is in != invert,
 * so add is the rows decided without a look that the request keeps. */
__global__ void __launch_bounds__(256)
k_plane_fcb(const uint4 *__restrict__ data, BucketFcArgs ba, SplitFcArgs sf,
            unsigned long long add,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  constexpr int UNR = 4;
  constexpr uint32_t R = 8;                        /* rows per 16 B */
  const bool inv = ba.invert != 0;
  unsigned long long cnt =
      (blockIdx.x == 0 && threadIdx.x == 0) ? add : 0ull;
  uint64_t vb[2] = {0, 0}, vn[2] = {0, 0};
  uint32_t l_lo_pk[2] = {0, 0}, l_span_pk[2] = {0, 0};
  #pragma unroll
  for (uint32_t i = 0; i < 2; i++)
    if (i < ba.n_slices && ba.end[i] > ba.beg[i]) {
      vb[i] = ba.beg[i] / R;
      vn[i] = (ba.end[i] + R - 1) / R - vb[i];
      /* [lo, lo + span] cut down to bucket h: not empty, h is a maybe bucket */
      const uint32_t b0 = ba.h[i] << 16, hi_end = sf.lo + sf.span;
      const uint32_t a = sf.lo > b0 ? sf.lo : b0;
      const uint32_t b = hi_end < (b0 | 0xFFFFu) ? hi_end : (b0 | 0xFFFFu);
      l_lo_pk[i] = fold_pack16(a & 0xFFFFu);
      l_span_pk[i] = fold_pack16(b - a);
    }
  const uint64_t n_vec = vn[0] + vn[1];
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  /* b0 = p0 - threadIdx.x, the block's first vector (uniform) */
  uint64_t b0 = (uint64_t)blockIdx.x * 256u * UNR;
  for (uint64_t p0 = b0 + threadIdx.x; p0 < n_vec; p0 += step, b0 += step) {
    uint4 v[UNR];
    /* the slice of the block's first and last vector (uniform) */
    const uint32_t s0 = b0 >= vn[0] ? 1u : 0u;
    const uint64_t e0 = b0 + 256u * UNR - 1;
    const uint32_t s1 = e0 >= vn[0] ? 1u : 0u;
    const uint64_t q0 = vb[s0] + (b0 - (s0 ? vn[0] : 0));   /* in bkt_lo */
    if (e0 < n_vec && s0 == s1 && q0 * R >= ba.beg[s0] &&
        (q0 + 256u * UNR) * R <= ba.end[s0]) {
      const uint4 *src = data + q0 + threadIdx.x;
      #pragma unroll
      for (int u = 0; u < UNR; u++) v[u] = src[(uint64_t)u * 256u];
      __builtin_amdgcn_sched_barrier(0);
      uint32_t acc = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++)
        acc = packed_out_acc(v[u], l_lo_pk[s0], l_span_pk[s0], acc);
      const uint32_t out = packed_sum(acc);
      cnt += inv ? out : UNR * R - out;
      continue;
    }
    uint64_t q[UNR];
    uint32_t sl[UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      const uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
      sl[u] = p >= vn[0] ? 1u : 0u;
      q[u] = vb[sl[u]] + (p - (sl[u] ? vn[0] : 0));
      v[u] = data[q[u]];
    }
    /* all four loads issue before the first is used */
    __builtin_amdgcn_sched_barrier(0);
    uint32_t c = 0;
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      if (p0 + (uint64_t)u * 256u >= n_vec) continue;
      const uint64_t beg = ba.beg[sl[u]], end = ba.end[sl[u]];
      const uint32_t h = ba.h[sl[u]];
      const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      #pragma unroll
      for (uint32_t j = 0; j < R; j++) {
        const uint64_t row = q[u] * R + j;
        const uint32_t l = (j & 1u) ? w[j / 2] >> 16 : w[j / 2] & 0xFFFFu;
        const bool keep = split_full_in(h, l, sf) != inv;
        c += (row >= beg && row < end && keep) ? 1u : 0u;
      }
    }
    cnt += c;
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

/* ---------------- two conditions over two columns -------------
 * count(*) WHERE cmp(a, ca) AND cmp(b, cb) over the narrow companions of both
 * columns. W is a side's width, 1, 2 or 4 = split, and WA <= WB (the host
 * orders the sides). A lane's unit is 16 consecutive rows, the same rows of
 * both planes: one 16 B vector of a 1-byte plane, two of a 2-byte plane or of
 * a split plane's halves. An iteration takes two units per lane, unit u of
 * lane t at b0 + 256 u + t, so a row mask is one word: unit u's row j is bit
 * 16 u + j, which is bit 8 k + j of a 2-byte side's vector k = 2 u + (j >> 3).
 * The helpers below take a side's vectors as an array of four; a 1-byte side
 * uses the first two. */

/* the index of a side's vector k, clamped to the plane's last vector */
template <int W>
__device__ __forceinline__ uint64_t
fc2_vec(const uint64_t (&q)[2], int k, uint64_t n_vec) {
  const uint64_t p = W == 1 ? q[k] : 2 * q[k >> 1] + (uint64_t)(k & 1);
  return min(p, n_vec - 1);
}

/* phase one of a side: in = the rows the loaded bytes put inside the
   interval, open = the rows they cannot decide (a split side's maybe and not
   sure). A 1- or 2-byte side decides every row by k_plane_fcn's test. */
template <int W>
__device__ __forceinline__ void
fc2_classify(const uint4 (&v)[4], const SplitFcArgs &sf, uint32_t &in,
             uint32_t &open) {
  in = 0;
  open = 0;
  #pragma unroll
  for (int k = 0; k < (W == 1 ? 2 : 4); k++) {
    const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
    if constexpr (W == 1) {
      #pragma unroll
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t n = (w[j / 4] >> (8u * (j % 4))) & 0xFFu;
        in |= ((n - sf.lo) <= sf.span ? 1u : 0u) << (16 * k + j);
      }
    } else {
      #pragma unroll
      for (uint32_t j = 0; j < 8; j++) {
        const uint32_t h = (j & 1u) ? w[j / 2] >> 16 : w[j / 2] & 0xFFFFu;
        if constexpr (W == 2) {
          in |= ((h - sf.lo) <= sf.span ? 1u : 0u) << (8 * k + j);
        } else {
          const bool m = split_maybe(h, sf), s = split_sure(h, sf);
          in |= (s ? 1u : 0u) << (8 * k + j);
          open |= (m && !s ? 1u : 0u) << (8 * k + j);
        }
      }
    }
  }
}

/* phase two of a split side: the low-half vectors that hold a needed row,
   every vector when 16 or more lanes of the wave (lanes, a ballot) need one:
   k_plane_fcs's dense rule */
__device__ __forceinline__ void
fc2_load_lo(const uint4 *__restrict__ lo, const uint64_t (&q)[2],
            uint64_t n_vec, uint32_t need, unsigned long long lanes,
            uint4 (&lv)[4]) {
  const bool dense = __popcll(lanes) >= 16;
  #pragma unroll
  for (int k = 0; k < 4; k++) {
    lv[k] = make_uint4(0, 0, 0, 0);
    if (dense || ((need >> (8 * k)) & 0xFFu))
      lv[k] = lo[fc2_vec<4>(q, k, n_vec)];
  }
}

/* the rows of a split side whose two halves pass the full test */
__device__ __forceinline__ uint32_t
fc2_full(const uint4 (&hv)[4], const uint4 (&lv)[4], const SplitFcArgs &sf) {
  uint32_t full = 0;
  #pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t wh[4] = {hv[k].x, hv[k].y, hv[k].z, hv[k].w};
    const uint32_t wl[4] = {lv[k].x, lv[k].y, lv[k].z, lv[k].w};
    #pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
      const uint32_t h = (j & 1u) ? wh[j / 2] >> 16 : wh[j / 2] & 0xFFFFu;
      const uint32_t l = (j & 1u) ? wl[j / 2] >> 16 : wl[j / 2] & 0xFFFFu;
      full |= (split_full_in(h, l, sf) ? 1u : 0u) << (8 * k + j);
    }
  }
  return full;
}

/* The kernel. Grid-stride over gridDim.x x 256 lanes x 32 rows; b0, the
 * block's first unit, is uniform, so every lane of a wave takes every
 * iteration and the ballots below are whole. All vectors of both sides issue
 * before the first is used; loads are clamped to each plane's last vector and
 * rows masked by n_rows (live), so the tail slack may be read and never
 * decides a row.
 * Phase one classifies both sides. A decided side keeps in ^ invert. A split
 * side's open rows need their low halves only where they are live and the
 * other side has not already rejected the row (an open row of the other side
 * counts as not rejected): need = open & live & (other.open | other.keep).
 * A wave without a needed row skips phase two; otherwise it loads the low
 * vectors that hold one (both sides' before either is used) and resolves the
 * needed rows with split_full_in. An open row that was not needed keeps its
 * provisional bit, which the other side's zero masks.
 * count += popc(keepA & keepB & live); the tail is fcn_block_count's. */
template <int WA, int WB>
__global__ void __launch_bounds__(256)
k_plane_fc2(const uint4 *__restrict__ a, const uint4 *__restrict__ a_lo,
            const uint4 *__restrict__ b, const uint4 *__restrict__ b_lo,
            uint64_t n_rows, SplitFcArgs sa, SplitFcArgs sb,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  static_assert(WA <= WB, "the host orders the sides");
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  const uint32_t inva = sa.invert ? ~0u : 0u, invb = sb.invert ? ~0u : 0u;
  const uint64_t n_units = (n_rows + 15) / 16;
  const uint64_t nva = WA == 1 ? n_units : (n_rows + 7) / 8;
  const uint64_t nvb = WB == 1 ? n_units : (n_rows + 7) / 8;
  const uint64_t step = (uint64_t)gridDim.x * 512u;
  unsigned long long cnt = 0;
  for (uint64_t b0 = (uint64_t)blockIdx.x * 512u; b0 < n_units; b0 += step) {
    const uint64_t q[2] = {b0 + threadIdx.x, b0 + 256u + threadIdx.x};
    uint4 va[4], vb[4];
    #pragma unroll
    for (int k = 0; k < (WA == 1 ? 2 : 4); k++)
      va[k] = a[fc2_vec<WA>(q, k, nva)];
    #pragma unroll
    for (int k = 0; k < (WB == 1 ? 2 : 4); k++)
      vb[k] = b[fc2_vec<WB>(q, k, nvb)];
    /* every load of both planes issues before the first is used */
    __builtin_amdgcn_sched_barrier(0);
    uint32_t live = 0;
    #pragma unroll
    for (int u = 0; u < 2; u++)
      if (q[u] < n_units) {
        const uint64_t left = n_rows - q[u] * 16u;
        live |= (left < 16u ? (1u << (uint32_t)left) - 1u : 0xFFFFu) << (16 * u);
      }
    uint32_t ina, opena, inb, openb;
    fc2_classify<WA>(va, sa, ina, opena);
    fc2_classify<WB>(vb, sb, inb, openb);
    uint32_t keepa = ina ^ inva, keepb = inb ^ invb;
    if constexpr (WB == 4) {                 /* WA <= WB: some side is split */
      const uint32_t needa = opena & live & (openb | keepb);   /* 0: WA < 4 */
      const uint32_t needb = openb & live & (opena | keepa);
      const unsigned long long la =
          WA == 4 ? __builtin_amdgcn_ballot_w64(needa != 0) : 0ull;
      const unsigned long long lb = __builtin_amdgcn_ballot_w64(needb != 0);
      if ((la | lb) != 0) {                  /* wave-uniform */
        uint4 wa[4], wb[4];
        if (WA == 4 && la != 0) fc2_load_lo(a_lo, q, nva, needa, la, wa);
        if (lb != 0) fc2_load_lo(b_lo, q, nvb, needb, lb, wb);
        __builtin_amdgcn_sched_barrier(0);
        if (WA == 4 && la != 0)
          keepa = (ina | (fc2_full(va, wa, sa) & needa)) ^ inva;
        if (lb != 0)
          keepb = (inb | (fc2_full(vb, wb, sb) & needb)) ^ invb;
      }
    }
    cnt += __popc(keepa & keepb & live);
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

/* IN-list filter+count over a narrow plane of 1 or 2 bytes per row (DESIGN
 * §9o). A stored n = v - base lies in [0, nmax], nmax < 2^(8 sizeof(T)), so
 * the list turns into a bitmap over that domain: 32 B for one byte, 8 KiB for
 * two. Each block zeroes its bitmap in LDS, then its lanes walk the slots of
 * the set image (global memory, 16 KiB at most) and for every key k with
 * (uint64)(k - base) <= nmax set bit k - base with an LDS atomic OR. The
 * difference is taken modulo 2^64 over the 64-bit patterns, which is exact
 * for either signedness: base + nmax does not wrap, so a key is a value of the
 * plane exactly when the difference is at most nmax.
 * After the barrier the block streams as k_plane_fcn does, 16 B = 16 or 8
 * rows per lane and load, UNR loads in flight, loads clamped to the last
 * vector and rows masked by n_rows. The row test is one LDS word read and a
 * shift, != invert; a byte of the tail slack indexes inside the bitmap
 * whatever it holds. Every row is a known int: no state, no ABSENT fill, no
 * parse error. The tail is fcn_block_count's: count slots, and
 * with a ticket the launch finalizes its request as k_plane_fcn does. */
template <typename T>
__global__ void __launch_bounds__(256)
k_plane_inb(const uint4 *__restrict__ data, uint64_t n_rows,
            const unsigned long long *__restrict__ tab, uint32_t n_slots,
            unsigned long long empty, unsigned long long base,
            unsigned long long nmax, uint32_t invert, uint32_t never,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  constexpr int UNR = COPR_PLANE_INB_UNR;
  constexpr uint32_t R = 16u / sizeof(T);          /* rows per 16 B */
  constexpr uint32_t PW = 4u / sizeof(T);          /* rows per 32-bit word */
  constexpr uint32_t BITS = 1u << (8 * sizeof(T));
  constexpr uint32_t WORDS = BITS / 32u;
  __shared__ uint32_t s_bm[WORDS];
  for (uint32_t i = threadIdx.x; i < WORDS; i += 256u) s_bm[i] = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_slots; i += 256u) {
    const unsigned long long k = tab[i];
    const unsigned long long d = k - base;
    if (k != empty && d <= nmax && d < BITS)
      atomicOr(&s_bm[(uint32_t)d >> 5], 1u << ((uint32_t)d & 31u));
  }
  __syncthreads();

  const bool inv = invert != 0;
  unsigned long long cnt = 0;
  const uint64_t n_vec = (n_rows + R - 1) / R;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256u * UNR + threadIdx.x;
       p0 < n_vec; p0 += step) {
    uint4 v[UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
      v[u] = data[p];
    }
    /* all four loads issue before the first is used */
    __builtin_amdgcn_sched_barrier(0);
    uint32_t c = 0;
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      const uint64_t p = p0 + (uint64_t)u * 256u;
      /* rows of this vector inside the plane: R except in the last vector */
      uint32_t live = 0;
      if (p < n_vec) {
        const uint64_t left = n_rows - p * R;
        live = left < R ? (uint32_t)left : R;
      }
      const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      #pragma unroll
      for (uint32_t j = 0; j < R; j++) {
        const uint32_t n =
            (w[j / PW] >> (8u * sizeof(T) * (j % PW))) & (BITS - 1u);
        const bool in = ((s_bm[n >> 5] >> (n & 31u)) & 1u) != 0;
        c += (j < live && in != inv) ? 1u : 0u;
      }
    }
    cnt += c;
  }
  if (never) cnt = 0;
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

/* IN-list filter+count over a split plane: k_plane_fcs's shape
 * with the list in the place of the range. A key can only equal a row whose
 * high half names the key's bucket (in_set.h, in_split_bucket), so the high
 * halves alone dismiss every row outside the flagged buckets.
 * Prologue, once per block: zero the bucket bitmap's words up to nmax >> 16
 * (8 KiB at most), then walk the image's slots, copy each to the LDS image
 * (dynamic, n_slots x 8 B, 16 KiB at most) and set its key's bucket bit with
 * an LDS atomic OR; one barrier.
 * Phase one reads 16 B = 8 rows of hi per lane and load, four loads in flight.
 * An iteration fully inside the plane counts its rows packed over the hull of
 * the flagged buckets (sa.hull_*_pk, two rows per instruction); a wave whose
 * ballot finds every row outside the hull reads no LDS. Otherwise each row's h
 * is tested against the bitmap, one LDS word and a shift: amb = the live rows
 * whose bucket is flagged. A row at or beyond n_rows is never open; the tail
 * slack may hold an h beyond the zeroed words, still inside the array.
 * Phase two is k_plane_fcs's: a wave-uniform ballot on amb, predicated lo
 * loads per vector in a sparse wave and unpredicated ones with 16 or more open
 * lanes, all before first use; each open row probes the LDS image with
 * base + ((h << 16) | l).
 * A launch with sa.none or never streams nothing (the launcher gives it one
 * block): NOT IN without a key in the domain keeps every row, the other forms
 * none. It still passes through the tail, so a one-dispatch request ends. */
__global__ void __launch_bounds__(256)
k_plane_ins(const uint4 *__restrict__ hi, const uint4 *__restrict__ lo,
            uint64_t n_rows, const unsigned long long *__restrict__ tab,
            uint32_t n_slots, unsigned long long empty,
            unsigned long long base, unsigned long long nmax, InSplitArgs sa,
            uint32_t invert, uint32_t never,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out,
            unsigned long long *__restrict__ stamp, unsigned long long seq) {
  const unsigned long long t_entry = fcn_entry_clock(stamp);
  constexpr int UNR = 4;
  constexpr uint32_t R = 8;                        /* rows per 16 B */
  __shared__ uint32_t s_bm[COPR_PLANE_INS_BM_WORDS];
  extern __shared__ uint64_t s_tab[];
  const bool inv = invert != 0;
  unsigned long long cnt = 0;
  /* kernel-uniform */
  const bool streams = !sa.none && !never;
  if (!streams) {
    if (inv && !never && blockIdx.x == 0 && threadIdx.x == 0) cnt = n_rows;
  } else {
    uint32_t bm_words = ((uint32_t)(nmax >> 16) >> 5) + 1u;
    if (bm_words > COPR_PLANE_INS_BM_WORDS) bm_words = COPR_PLANE_INS_BM_WORDS;
    for (uint32_t i = threadIdx.x; i < bm_words; i += 256u) s_bm[i] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += 256u) {
      const uint64_t k = tab[i];
      s_tab[i] = k;
      uint32_t b;
      if (in_split_bucket(k, empty, base, nmax, &b))
        atomicOr(&s_bm[b >> 5], 1u << (b & 31u));
    }
    __syncthreads();
  }
  const uint32_t in_mask = n_slots - 1u;
  const uint64_t n_vec = streams ? (n_rows + R - 1) / R : 0;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  /* b0 = p0 - threadIdx.x, the block's first vector, kept beside p0 so that
     the compiler sees it is the same in every lane */
  uint64_t b0 = (uint64_t)blockIdx.x * 256u * UNR;
  for (uint64_t p0 = b0 + threadIdx.x; p0 < n_vec; p0 += step, b0 += step) {
    uint4 v[UNR];
    /* one bit per row, vector u in bits 8u .. 8u + 7 */
    uint32_t livem = ~0u, amb = 0;
    bool classify = true;
    if ((b0 + 256u * UNR) * R <= n_rows) {
      #pragma unroll
      for (int u = 0; u < UNR; u++) v[u] = hi[p0 + (uint64_t)u * 256u];
      /* all four loads issue before the first is used */
      __builtin_amdgcn_sched_barrier(0);
      uint32_t acc = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++)
        acc = packed_out_acc(v[u], sa.hull_lo_pk, sa.hull_span_pk, acc);
      /* rows outside the hull; a wave with none inside it is done */
      classify =
          __builtin_amdgcn_ballot_w64(packed_sum(acc) != UNR * R) != 0;
    } else {
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
        v[u] = hi[p];
      }
      /* all four loads issue before the first is used */
      __builtin_amdgcn_sched_barrier(0);
      livem = 0;
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        const uint64_t p = p0 + (uint64_t)u * 256u;
        uint32_t live = 0;
        if (p < n_vec) {
          const uint64_t left = n_rows - p * R;
          live = left < R ? (uint32_t)left : R;
        }
        livem |= ((1u << live) - 1u) << (u * R);
      }
    }
    if (classify) {             /* wave-uniform */
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        #pragma unroll
        for (uint32_t j = 0; j < R; j++) {
          const uint32_t h = (j & 1u) ? w[j / 2] >> 16 : w[j / 2] & 0xFFFFu;
          amb |= ((s_bm[h >> 5] >> (h & 31u)) & 1u) << (u * R + j);
        }
      }
      amb &= livem;
    }
    uint32_t in = 0;
    const unsigned long long open_lanes =
        __builtin_amdgcn_ballot_w64(amb != 0);
    if (open_lanes != 0) {
      uint4 lv[UNR];
      if (__popcll(open_lanes) >= 16) {
        /* dense (wave-uniform): every lane loads its four vectors,
           unpredicated and coalesced */
        #pragma unroll
        for (int u = 0; u < UNR; u++)
          lv[u] = lo[min(p0 + (uint64_t)u * 256u, n_vec - 1)];
      } else {
        #pragma unroll
        for (int u = 0; u < UNR; u++) {
          lv[u] = make_uint4(0, 0, 0, 0);
          if ((amb >> (u * R)) & 0xFFu)
            lv[u] = lo[min(p0 + (uint64_t)u * 256u, n_vec - 1)];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      #pragma unroll
      for (int u = 0; u < UNR; u++) {
        if (!((amb >> (u * R)) & 0xFFu)) continue;
        const uint32_t wh[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        const uint32_t wl[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w};
        #pragma unroll
        for (uint32_t j = 0; j < R; j++) {
          if (!((amb >> (u * R + j)) & 1u)) continue;
          const uint32_t h = (j & 1u) ? wh[j / 2] >> 16 : wh[j / 2] & 0xFFFFu;
          const uint32_t l = (j & 1u) ? wl[j / 2] >> 16 : wl[j / 2] & 0xFFFFu;
          in += in_set_probe(s_tab, in_mask, empty,
                             base + (((uint64_t)h << 16) | l)) ? 1u : 0u;
        }
      }
    }
    cnt += inv ? __popc(livem) - in : in;
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out, stamp, t_entry, seq);
}

int dev_plane_inn_launch(const DevRegion::ColPlane &p, const ScanPlan &plan,
                         const InFcArgs &fa, const InSplitArgs &sa,
                         uint64_t n_rows, unsigned long long *d_cnt,
                         uint32_t n_slots, unsigned int *d_ticket,
                         unsigned long long *h_out,
                         unsigned long long *d_stamp, unsigned long long seq,
                         uint32_t grid_cap, uint32_t *grid_out,
                         void *stream) {
  /* dev_plane_fcn_launch's checks on the one-dispatch arguments */
  if (d_stamp && d_ticket &&
      d_stamp != (unsigned long long *)d_ticket + COPR_FCN_STAMP_WORD)
    return -1;
  if (!p.nar || (d_ticket && (!h_out || !seq)) || !n_slots || n_slots > 64 ||
      (n_slots & (n_slots - 1)) || (p.nar_w == 4) != (p.nar_lo_off != 0))
    return -1;
  /* and k_plane_inb's on the plane and the image */
  if ((p.nar_w != 1 && p.nar_w != 2 && p.nar_w != 4) ||
      p.nar_nmax >= (1ull << (8 * p.nar_w)) || !plan.in_tab ||
      plan.in_mask + 1 < COPR_IN_MIN_SLOTS ||
      plan.in_mask + 1 > COPR_IN_MAX_SLOTS ||
      (plan.in_mask & (plan.in_mask + 1)))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  const bool split = p.nar_w == 4;
  /* a split plane streams its 2-byte high halves */
  const uint32_t rows_per_vec = split ? 8u : 16u / p.nar_w;
  const uint64_t n_vec = (n_rows + rows_per_vec - 1) / rows_per_vec;
  /* dev_plane_fcn_launch's grids: 2048 blocks = 8 per CU, and over a split
     plane 768 = 3 per CU while phase one is the work, as in k_plane_fcs. Once
     a wave's iteration (64 lanes x 32 rows) expects an open row, the probes'
     latency is the work and more waves hide it: 2048 again. Measured at three
     lists: tuned figures, not rules; COPR_IN_GRID overrides
     them. A finalizing launch needs a block even over no rows, and a launch
     that does not stream needs no more than one */
  uint64_t nb = (n_vec + 256u * COPR_PLANE_INB_UNR - 1) /
                (256u * COPR_PLANE_INB_UNR);
  const bool light = split && (uint64_t)sa.flagged * 2048u < sa.buckets;
  const uint64_t cap = grid_cap ? grid_cap : light ? 768u : 2048u;
  if (nb > cap) nb = cap;
  if (!nb || (split && (sa.none || fa.never))) nb = 1;
  if (grid_out) *grid_out = (uint32_t)nb;
  const uint4 *data = (const uint4 *)p.nar;
  const uint32_t mask = n_slots - 1;
  const uint32_t in_slots = plan.in_mask + 1;
  const unsigned long long base = (unsigned long long)p.nar_base;
  const unsigned long long nmax = (unsigned long long)p.nar_nmax;
  if (p.nar_w == 1)
    hipLaunchKernelGGL(k_plane_inb<uint8_t>, dim3((uint32_t)nb), dim3(256), 0,
                       s, data, n_rows, plan.in_tab, in_slots, plan.in_empty,
                       base, nmax, fa.invert, fa.never, d_cnt, mask, d_ticket,
                       h_out, d_stamp, seq);
  else if (p.nar_w == 2)
    hipLaunchKernelGGL(k_plane_inb<uint16_t>, dim3((uint32_t)nb), dim3(256), 0,
                       s, data, n_rows, plan.in_tab, in_slots, plan.in_empty,
                       base, nmax, fa.invert, fa.never, d_cnt, mask, d_ticket,
                       h_out, d_stamp, seq);
  else
    hipLaunchKernelGGL(k_plane_ins, dim3((uint32_t)nb), dim3(256),
                       (size_t)in_slots * 8, s, data,
                       (const uint4 *)((const uint8_t *)p.nar + p.nar_lo_off),
                       n_rows, plan.in_tab, in_slots, plan.in_empty, base,
                       nmax, sa, fa.invert, fa.never, d_cnt, mask, d_ticket,
                       h_out, d_stamp, seq);
  return (int)hipGetLastError();
}

int dev_plane_fcn_launch(const DevRegion::ColPlane &p, const NarrowFcArgs &nf,
                         const SplitFcArgs &sf, const BucketFcArgs *ba,
                         uint64_t n_rows, unsigned long long *d_cnt,
                         uint32_t n_slots, unsigned int *d_ticket,
                         unsigned long long *h_out,
                         unsigned long long *d_stamp, unsigned long long seq,
                         uint32_t grid_cap, uint32_t *grid_out,
                         void *stream) {
  /* a stamp is taken back by a finalizing launch alone, and its word sits
     behind the ticket */
  if (d_stamp && d_ticket &&
      d_stamp != (unsigned long long *)d_ticket + COPR_FCN_STAMP_WORD)
    return -1;
  if (!p.nar || (d_ticket && (!h_out || !seq)) || !n_slots || n_slots > 64 ||
      (n_slots & (n_slots - 1)) || (p.nar_w == 4) != (p.nar_lo_off != 0))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  /* a split plane streams its 2-byte high halves */
  const uint32_t rows_per_vec = p.nar_lo_off ? 8u : 16u / p.nar_w;
  const uint64_t n_vec = (n_rows + rows_per_vec - 1) / rows_per_vec;
  /* 2048 blocks = 8 per CU, each lane with 4 x 16 B in flight. k_plane_fcs,
     whose packed count leaves a wave little to do per byte, measured fastest
     at 768 = 3 per CU on the one shape tried: the benchmark's column at 100 M
     and 150 M rows, plain and with every row through both halves (DESIGN
     §9l). It is a tuned figure, not a rule; COPR_NARROW_GRID overrides it. A
     finalizing launch needs at least one block even over no rows */
  uint64_t nb = (n_vec + 256u * 4 - 1) / (256u * 4);
  const uint64_t cap = grid_cap ? grid_cap : p.nar_lo_off ? 768u : 2048u;
  if (nb > cap) nb = cap;
  if (!nb) nb = 1;
  if (grid_out) *grid_out = (uint32_t)nb;
  const uint4 *data = (const uint4 *)p.nar;
  const uint32_t mask = n_slots - 1;
  if (ba) {
    /* the bucket index: one block per 8192 slice rows, at least
       one, under the split plane's cap. The slices are checked against the
       plane once more here: the kernel trusts them */
    if (!p.bkt_lo || !p.nar_lo_off || ba->n_slices > 2 || ba->sure > n_rows)
      return -1;
    uint64_t slice_rows = 0, vecs = 0;
    for (uint32_t i = 0; i < ba->n_slices; i++) {
      if (ba->beg[i] > ba->end[i] || ba->end[i] > n_rows ||
          ba->h[i] >= COPR_N_BUCKETS)
        return -1;
      slice_rows += ba->end[i] - ba->beg[i];
      if (ba->end[i] > ba->beg[i])
        vecs += (ba->end[i] + 7) / 8 - ba->beg[i] / 8;
    }
    if (ba->sure + slice_rows > n_rows) return -1;
    uint64_t bb = (vecs + 256u * 4 - 1) / (256u * 4);
    if (bb > cap) bb = cap;
    if (!bb) bb = 1;
    /* a launch that opens and finalizes takes one block for up to two
       iterations (2048 vectors): the solo tail's second load round trip
       is shorter than the ticketed tail's three atomic ones. Measured at
       8193 and 16384 slice rows, behind from 32768 on;
       COPR_NARROW_GRID=2 still gives two blocks */
    if (!grid_cap && d_stamp && d_ticket && bb == 2) bb = 1;
    if (grid_out) *grid_out = (uint32_t)bb;
    const unsigned long long add =
        ba->invert ? n_rows - ba->sure - slice_rows : ba->sure;
    hipLaunchKernelGGL(k_plane_fcb, dim3((uint32_t)bb), dim3(256), 0, s,
                       (const uint4 *)p.bkt_lo, *ba, sf, add, d_cnt, mask,
                       d_ticket, h_out, d_stamp, seq);
    return (int)hipGetLastError();
  }
  switch (p.nar_w) {
    case 1:
      hipLaunchKernelGGL(k_plane_fcn<uint8_t>, dim3((uint32_t)nb), dim3(256),
                         0, s, data, n_rows, nf, d_cnt, mask, d_ticket, h_out,
                         d_stamp, seq);
      break;
    case 2:
      hipLaunchKernelGGL(k_plane_fcn<uint16_t>, dim3((uint32_t)nb), dim3(256),
                         0, s, data, n_rows, nf, d_cnt, mask, d_ticket, h_out,
                         d_stamp, seq);
      break;
    case 4:
      hipLaunchKernelGGL(k_plane_fcs, dim3((uint32_t)nb), dim3(256), 0, s, data,
                         (const uint4 *)((const uint8_t *)p.nar + p.nar_lo_off),
                         n_rows, sf, d_cnt, mask, d_ticket, h_out, d_stamp, seq);
      break;
    default:
      return -1;
  }
  return (int)hipGetLastError();
}

int dev_plane_fc2_launch(const DevRegion::ColPlane &pa, const SplitFcArgs &sa,
                         const DevRegion::ColPlane &pb, const SplitFcArgs &sb,
                         uint64_t n_rows, unsigned long long *d_cnt,
                         uint32_t n_slots, unsigned int *d_ticket,
                         unsigned long long *h_out,
                         unsigned long long *d_stamp, unsigned long long seq,
                         uint32_t grid_cap, uint32_t *grid_out,
                         void *stream) {
  /* dev_plane_fcn_launch's checks on the one-dispatch arguments */
  if (d_stamp && d_ticket &&
      d_stamp != (unsigned long long *)d_ticket + COPR_FCN_STAMP_WORD)
    return -1;
  if (!pa.nar || !pb.nar || (d_ticket && (!h_out || !seq)) || !n_slots ||
      n_slots > 64 || (n_slots & (n_slots - 1)) ||
      (pa.nar_w == 4) != (pa.nar_lo_off != 0) ||
      (pb.nar_w == 4) != (pb.nar_lo_off != 0) || pa.nar_w > pb.nar_w)
    return -1;
  hipStream_t s = (hipStream_t)stream;
  /* one block per 256 lanes x 32 rows, under dev_plane_fcn_launch's caps: 2048
     blocks, 768 with a split side. Starting figures, not measured for this
     kernel; COPR_NARROW_GRID overrides them. A finalizing launch
     needs a block even over no rows */
  const uint64_t n_units = (n_rows + 15) / 16;
  uint64_t nb = (n_units + 511) / 512;
  const uint64_t cap = grid_cap ? grid_cap : pb.nar_lo_off ? 768u : 2048u;
  if (nb > cap) nb = cap;
  if (!nb) nb = 1;
  if (grid_out) *grid_out = (uint32_t)nb;
  const uint4 *a = (const uint4 *)pa.nar, *b = (const uint4 *)pb.nar;
  const uint4 *a_lo = (const uint4 *)((const uint8_t *)pa.nar + pa.nar_lo_off);
  const uint4 *b_lo = (const uint4 *)((const uint8_t *)pb.nar + pb.nar_lo_off);
  const uint32_t mask = n_slots - 1;
  #define COPR_FC2(WA, WB)                                                   \
    hipLaunchKernelGGL((k_plane_fc2<WA, WB>), dim3((uint32_t)nb), dim3(256), \
                       0, s, a, a_lo, b, b_lo, n_rows, sa, sb, d_cnt, mask,  \
                       d_ticket, h_out, d_stamp, seq)
  switch (pa.nar_w * 8 + pb.nar_w) {
    case 1 * 8 + 1: COPR_FC2(1, 1); break;
    case 1 * 8 + 2: COPR_FC2(1, 2); break;
    case 1 * 8 + 4: COPR_FC2(1, 4); break;
    case 2 * 8 + 2: COPR_FC2(2, 2); break;
    case 2 * 8 + 4: COPR_FC2(2, 4); break;
    case 4 * 8 + 4: COPR_FC2(4, 4); break;
    default: return -1;
  }
  #undef COPR_FC2
  return (int)hipGetLastError();
}

}  // namespace copr
