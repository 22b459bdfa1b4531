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
   inside both planes' tail slack. */
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
  void *nar = nullptr;
  if (hipMalloc(&nar, cost + 2048) != hipSuccess) {
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
      hipLaunchKernelGGL(k_plane_narrow<uint32_t>, dim3(grid), dim3(256), 0, s,
                         src, rgn.n_kv, base, (NarrowQuad<uint32_t> *)nar);
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
  p->nar_base = base;
  p->nar_nmax = nmax;
  p->nar_verdict = NAR_BUILT;
  rgn.plane_bytes += cost;
  if (built) (*built)++;
  return p;
}

/* Filter+count over a narrow plane. Each lane loads 16 B = 16 / sizeof(T)
 * rows, UNR loads in flight, grid-stride; the row test is the 32-bit form of
 * k_plane_fc's (narrow_fc_fold, plane_fold.h). Every row is a known int, so
 * there is no state, no ABSENT fill and no parse error. Loads are clamped to
 * the last vector and rows masked by n_rows, as in k_plane_fc; the last
 * vector may read up to 15 B into the tail slack.
 * The block's count goes to one of slot_mask + 1 count words, each on a
 * 128 B line of its own, chosen by block index: thousands of adds to one word
 * queue up at the end of the launch, spread over 64 they do
 * not.
 * With a ticket the launch finalizes the request: lane 0 of each block draws
 * a ticket once its add has returned, and the block that draws the last one
 * collects the count words, hands the total to the host and leaves words and
 * ticket zero for the next request. Only atomics touch these words, so no
 * cache has to be written back or invalidated. */
template <typename T>
__global__ void __launch_bounds__(256)
k_plane_fcn(const uint4 *__restrict__ data, uint64_t n_rows, NarrowFcArgs nf,
            unsigned long long *__restrict__ cnt_out, uint32_t slot_mask,
            unsigned int *__restrict__ ticket,
            unsigned long long *__restrict__ h_out) {
  constexpr int UNR = 4;
  constexpr uint32_t R = 16u / sizeof(T);          /* rows per 16 B */
  constexpr uint32_t PW = 4u / sizeof(T);          /* rows per 32-bit word */
  __shared__ unsigned long long s_cnt[4];
  __shared__ unsigned int s_last;
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

int dev_plane_fcn_launch(const DevRegion::ColPlane &p, const NarrowFcArgs &nf,
                         uint64_t n_rows, unsigned long long *d_cnt,
                         uint32_t n_slots, unsigned int *d_ticket,
                         unsigned long long *h_out, uint32_t grid_cap,
                         void *stream) {
  if (!p.nar || (d_ticket && !h_out) || !n_slots || n_slots > 64 ||
      (n_slots & (n_slots - 1)))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t rows_per_vec = 16u / p.nar_w;
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
      hipLaunchKernelGGL(k_plane_fcn<uint32_t>, dim3((uint32_t)nb), dim3(256),
                         0, s, data, n_rows, nf, d_cnt, mask, d_ticket, h_out);
      break;
    default:
      return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace copr
