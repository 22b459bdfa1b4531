/* narrow_planes.hip — narrow companions of the decoded column planes and the
 * filter+count kernel over them. The wide planes, their build
 * and their consumers live in kernels.hip. */
#include <hip/hip_runtime.h>
#include "copr_internal.h"

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

const DevRegion::ColPlane *dev_colplane_narrow(DevRegion &rgn, int64_t col_id,
                                               uint64_t budget_bytes,
                                               hipStream_t s, uint64_t *built) {
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
 * collects the count words, hands the total to the host and leaves words and
 * ticket zero for the next request. Only atomics touch these words, so no
 * cache has to be written back or invalidated. */
__device__ __forceinline__ void
fcn_block_count(unsigned long long cnt, unsigned long long *__restrict__ cnt_out,
                uint32_t slot_mask, unsigned int *__restrict__ ticket,
                unsigned long long *__restrict__ h_out) {
  __shared__ unsigned long long s_cnt[4];
  __shared__ unsigned int s_last;
  for (int off = 32; off > 0; off >>= 1)
    cnt += (unsigned long long)__shfl_down((long long)cnt, off, 64);
  if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long b = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    unsigned long long *slot =
        cnt_out + (size_t)(blockIdx.x & slot_mask) * COPR_FCN_SLOT_STRIDE;
    unsigned int last = 0;
    if (!ticket) {
      if (b) atomicAdd(slot, b);
    } else {
      if (b) {
        /* the add has been performed once its old value is back */
        unsigned long long old = __hip_atomic_fetch_add(
            slot, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" :: "v"(old) : "memory");
      }
      unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
      last = t == gridDim.x - 1 ? 1u : 0u;
    }
    s_last = last;
  }
  if (!ticket) return;
  __syncthreads();
  if (!s_last || threadIdx.x >= 64u) return;
  /* every block's add returned before its ticket was drawn, and this block
     drew the last ticket: the words are final */
  unsigned long long tot = 0;
  if (threadIdx.x <= slot_mask)
    tot = __hip_atomic_exchange(
        cnt_out + (size_t)threadIdx.x * COPR_FCN_SLOT_STRIDE, 0ull,
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int off = 32; off > 0; off >>= 1)
    tot += (unsigned long long)__shfl_down((long long)tot, off, 64);
  if (threadIdx.x == 0) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *(volatile unsigned long long *)h_out = tot;
    __threadfence_system();
  }
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
            unsigned long long *__restrict__ h_out) {
  constexpr int UNR = 4;
  constexpr uint32_t R = 16u / sizeof(T);          /* rows per 16 B */
  constexpr uint32_t PW = 4u / sizeof(T);          /* rows per 32-bit word */
  const bool inv = nf.invert != 0;
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
        uint32_t n = w[j / PW];
        if (sizeof(T) < 4)
          n = (n >> (8u * sizeof(T) * (j % PW))) & (uint32_t)(T)~(T)0;
        const bool keep = ((n - nf.lo) <= nf.span) != inv;
        c += (j < live && keep) ? 1u : 0u;
      }
    }
    cnt += c;
  }
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out);
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
 * the launch reads n_rows x 4 bytes, as k_plane_fcn<uint32_t> did. */
__global__ void __launch_bounds__(256)
k_plane_fcs(const uint4 *__restrict__ hi, const uint4 *__restrict__ lo,
            uint64_t n_rows, SplitFcArgs sf,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out) {
  constexpr int UNR = 4;
  constexpr uint32_t R = 8;                        /* rows per 16 B */
  const bool inv = sf.invert != 0;
  unsigned long long cnt = 0;
  const uint64_t n_vec = (n_rows + R - 1) / R;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256u * UNR + threadIdx.x;
       p0 < n_vec; p0 += step) {
    uint4 v[UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_vec - 1);
      v[u] = hi[p];
    }
    /* all four loads issue before the first is used */
    __builtin_amdgcn_sched_barrier(0);
    /* one bit per row, vector u in bits 8u .. 8u + 7 */
    uint32_t livem = 0, maybe = 0, sure = 0;
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      const uint64_t p = p0 + (uint64_t)u * 256u;
      uint32_t live = 0;
      if (p < n_vec) {
        const uint64_t left = n_rows - p * R;
        live = left < R ? (uint32_t)left : R;
      }
      livem |= ((1u << live) - 1u) << (u * R);
      const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      #pragma unroll
      for (uint32_t j = 0; j < R; j++) {
        const uint32_t h = (j & 1u) ? w[j / 2] >> 16 : w[j / 2] & 0xFFFFu;
        maybe |= (split_maybe(h, sf) ? 1u : 0u) << (u * R + j);
        sure |= (split_sure(h, sf) ? 1u : 0u) << (u * R + j);
      }
    }
    uint32_t in = __popc(sure & livem);
    const uint32_t amb = maybe & ~sure & livem;
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
  fcn_block_count(cnt, cnt_out, slot_mask, ticket, h_out);
}

int dev_plane_fcn_launch(const DevRegion::ColPlane &p, const NarrowFcArgs &nf,
                         const SplitFcArgs &sf, uint64_t n_rows,
                         unsigned long long *d_cnt,
                         uint32_t n_slots, unsigned int *d_ticket,
                         unsigned long long *h_out, uint32_t grid_cap,
                         void *stream) {
  if (!p.nar || (d_ticket && !h_out) || !n_slots || n_slots > 64 ||
      (n_slots & (n_slots - 1)) || (p.nar_w == 4) != (p.nar_lo_off != 0))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  /* a split plane streams its 2-byte high halves */
  const uint32_t rows_per_vec = p.nar_lo_off ? 8u : 16u / p.nar_w;
  const uint64_t n_vec = (n_rows + rows_per_vec - 1) / rows_per_vec;
  /* 2048 blocks = 8 per CU, each lane with 4 x 16 B in flight; a finalizing
     launch needs at least one block even over no rows */
  uint64_t nb = (n_vec + 256u * 4 - 1) / (256u * 4);
  const uint64_t cap = grid_cap ? grid_cap : 2048u;
  if (nb > cap) nb = cap;
  if (!nb) nb = 1;
  const uint4 *data = (const uint4 *)p.nar;
  const uint32_t mask = n_slots - 1;
  switch (p.nar_w) {
    case 1:
      hipLaunchKernelGGL(k_plane_fcn<uint8_t>, dim3((uint32_t)nb), dim3(256),
                         0, s, data, n_rows, nf, d_cnt, mask, d_ticket, h_out);
      break;
    case 2:
      hipLaunchKernelGGL(k_plane_fcn<uint16_t>, dim3((uint32_t)nb), dim3(256),
                         0, s, data, n_rows, nf, d_cnt, mask, d_ticket, h_out);
      break;
    case 4:
      hipLaunchKernelGGL(k_plane_fcs, dim3((uint32_t)nb), dim3(256), 0, s, data,
                         (const uint4 *)((const uint8_t *)p.nar + p.nar_lo_off),
                         n_rows, sf, d_cnt, mask, d_ticket, h_out);
      break;
    default:
      return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace copr
