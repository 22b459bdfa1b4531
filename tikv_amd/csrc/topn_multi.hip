/* topn_multi.hip — TopN over several order-by columns.
 *
 * keep flags (the scan path's extract pass) -> kept row ids -> order key 0 as
 * (rank, u) composites (topn_keys.h) -> stable radix sort -> candidate cut at
 * position take - 1 -> keys 1..K-1 for the c candidates only -> stable LSD
 * passes over the candidates -> the first take row ids and their key values.
 * Everything after the cut scales with c, not with the kept row count m.
 * The keep pass and k_topn_keys need the row parsers and live in kernels.hip. */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "copr_internal.h"

#include <algorithm>

namespace copr {

__global__ void __launch_bounds__(256)
k_tm_flags(const uint8_t *__restrict__ st, uint32_t *__restrict__ f,
           uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = st[i] ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
k_tm_scatter_rows(const uint8_t *__restrict__ st,
                  const uint64_t *__restrict__ pos, uint64_t n, uint64_t m,
                  uint32_t *__restrict__ rows) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !st[i]) return;
  uint64_t p = pos[i];
  if (p < m) rows[p] = (uint32_t)i;
}

__global__ void __launch_bounds__(256)
k_tm_iota(uint32_t *__restrict__ idx, uint64_t cnt) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) idx[i] = (uint32_t)i;
}

/* out[i] = src[perm[i]]; every perm entry indexes src (callers pass
   permutations of, or prefixes of permutations of, src's index range) */
template <typename TI, typename TO>
__global__ void __launch_bounds__(256)
k_tm_gather(const TI *__restrict__ src, const uint32_t *__restrict__ perm,
            uint64_t cnt, TO *__restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) out[i] = (TO)src[perm[i]];
}

/* candidate count from the primary composites and their sorted order (one
   lane: a binary search of ~log2(m) dependent loads) */
__global__ void k_tm_cut(const uint8_t *__restrict__ rank,
                         const unsigned long long *__restrict__ u,
                         const uint32_t *__restrict__ perm, uint64_t m,
                         uint64_t take, unsigned long long *__restrict__ c) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *c = topn_cut(rank, u, perm, m, take);
}

/* key 0 from what the keep pass already parsed (its group slot): right when
   the column has no default, so that an absent cell is NULL, which is how
   the extract pass reports it (st 1 = kept, NULL or absent; 2 = value) */
__global__ void __launch_bounds__(256)
k_tm_key0_extract(const uint8_t *__restrict__ st,
                  const int64_t *__restrict__ gkey,
                  const uint32_t *__restrict__ rows, uint64_t cnt, TopnKey key,
                  unsigned long long *__restrict__ u_out,
                  uint8_t *__restrict__ rank_out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t row = rows[i];
  uint8_t rk;
  unsigned long long u;
  topn_key_encode(gkey[row], st[row] != 2, key.uns != 0, key.desc != 0, &rk, &u);
  u_out[i] = u;
  rank_out[i] = rk;
}

/* seen |= 1 << rank over all rows: 3 = both ranks occur, so the rank bit
   takes part in the order */
__global__ void __launch_bounds__(256)
k_tm_rank_seen(const uint8_t *__restrict__ rank, uint64_t cnt,
               unsigned int *__restrict__ seen) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned int v = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt;
       i += stride)
    v |= 1u << (rank[i] & 1u);
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_down(v, off, 64);
  if ((threadIdx.x & 63u) == 0 && v) atomicOr(seen, v);
}

/* 1 where a new run of equal primary composites starts (never at 0), so the
   inclusive sum numbers the runs from 0 in ascending order */
__global__ void __launch_bounds__(256)
k_tm_seg_flags(const uint8_t *__restrict__ rank,
               const unsigned long long *__restrict__ u, uint64_t cnt,
               uint32_t *__restrict__ f) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  f[i] = (i > 0 && (rank[i] != rank[i - 1] || u[i] != u[i - 1])) ? 1u : 0u;
}

template <typename TI, typename TO>
static void tm_gather(const TI *src, const uint32_t *perm, uint64_t cnt,
                      TO *out, hipStream_t s) {
  if (!cnt) return;
  hipLaunchKernelGGL((k_tm_gather<TI, TO>), dim3((uint32_t)((cnt + 255) / 256)),
                     dim3(256), 0, s, src, perm, cnt, out);
}

int dev_topn_multi_select(const ScanPlan &plan, const DevRegion &rgn,
                          uint64_t take, const TopnKey *keys, int n_keys,
                          void *stream, std::vector<uint32_t> *winners,
                          std::vector<int64_t> *key_vals,
                          std::vector<uint8_t> *key_nulls, uint64_t *kept,
                          uint64_t *cands) {
  hipStream_t s = (hipStream_t)stream;
  const uint64_t n = rgn.n_kv;
  winners->clear();
  for (int k = 0; k < n_keys; k++) {
    key_vals[k].clear();
    key_nulls[k].clear();
  }
  *kept = 0;
  *cands = 0;
  if (n_keys < 1 || n_keys > COPR_TOPN_MAX_KEYS || n > 0x7FFFFFFFull) return -1;
  if (!n || !take) return 0;

  std::vector<void *> bufs;
  void *tmp = nullptr;
  size_t tmpb = 0;
  bool oom = false;
  auto dalloc = [&](size_t bytes) -> void * {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) {
      oom = true;
      return nullptr;
    }
    bufs.push_back(p);
    return p;
  };
  auto freeall = [&]() {
    for (void *p : bufs) hipFree(p);
    bufs.clear();
    hipFree(tmp);
    tmp = nullptr;
  };
  auto need_tmp = [&](size_t tb) -> bool {
    if (tb <= tmpb) return true;
    hipFree(tmp);
    tmp = nullptr;
    tmpb = 0;
    if (hipMalloc(&tmp, tb) != hipSuccess) return false;
    tmpb = tb;
    return true;
  };
  auto blocks_of = [](uint64_t cnt) { return dim3((uint32_t)((cnt + 255) / 256)); };

  /* ---- 1. keep flags ---- */
  uint8_t *st = (uint8_t *)dalloc(n);
  int64_t *gkey = (int64_t *)dalloc(n * 8);
  uint32_t *f32 = (uint32_t *)dalloc(n * 4 + 4);
  uint64_t *pos = (uint64_t *)dalloc(n * 8 + 8);
  unsigned int *d_err = (unsigned int *)dalloc(4);
  unsigned long long *d_c = (unsigned long long *)dalloc(8);
  unsigned int *d_seen = (unsigned int *)dalloc(4);
  if (oom) { freeall(); return -2; }
  hipError_t e = hipMemsetAsync(d_err, 0, 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_seen, 0, 4, s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (dev_topn_keep_flags(plan, rgn, st, gkey, d_err, s)) { freeall(); return -1; }
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  /* ---- kept row ids, in source order ---- */
  hipLaunchKernelGGL(k_tm_flags, blocks_of(n), dim3(256), 0, s, st, f32, n);
  size_t tb = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tb, f32, pos, (int)n, s);
  if (!need_tmp(tb)) { freeall(); return -2; }
  if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, f32, pos, (int)n, s) != hipSuccess) {
    freeall();
    return -1;
  }
  uint64_t m = 0;
  uint32_t lf = 0;
  e = hipMemcpyAsync(&m, pos + (n - 1), 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&lf, f32 + (n - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  m += lf;
  *kept = m;
  if (!m) { freeall(); return 0; }

  uint32_t *rows = (uint32_t *)dalloc(m * 4);
  unsigned long long *u0 = (unsigned long long *)dalloc(m * 8);
  uint8_t *r0 = (uint8_t *)dalloc(m);
  uint32_t *idxA = (uint32_t *)dalloc(m * 4);
  uint32_t *idxB = (uint32_t *)dalloc(m * 4);
  unsigned long long *kA = (unsigned long long *)dalloc(m * 8);
  unsigned long long *kB = (unsigned long long *)dalloc(m * 8);
  if (oom) { freeall(); return -2; }
  hipLaunchKernelGGL(k_tm_scatter_rows, blocks_of(n), dim3(256), 0, s, st, pos,
                     n, m, rows);

  /* ---- 2. primary key: from the keep pass's own parse when an absent cell
     is NULL, else (column default) a pass of its own over the row bytes ---- */
  if (keys[0].missing_null) {
    hipLaunchKernelGGL(k_tm_key0_extract, blocks_of(m), dim3(256), 0, s, st,
                       gkey, rows, m, keys[0], u0, r0);
  } else if (dev_topn_keys_launch(rgn, rows, m, keys[0], u0, r0, d_err, s)) {
    freeall();
    return -1;
  }
  hipLaunchKernelGGL(k_tm_rank_seen,
                     dim3((uint32_t)std::min<uint64_t>((m + 255) / 256, 2048)),
                     dim3(256), 0, s, r0, m, d_seen);
  unsigned int h_seen = 0;
  e = hipMemcpyAsync(&h_seen, d_seen, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }

  /* one stable LSD pass: order idxA by key[idxA[i]] (low end_bit bits) */
  auto sort_by = [&](const unsigned long long *kin, uint64_t cnt,
                     int end_bit) -> int {
    size_t b = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, b, kin, kB, idxA, idxB,
                                       (int)cnt, 0, end_bit, s);
    if (!need_tmp(b)) return -2;
    if (hipcub::DeviceRadixSort::SortPairs(tmp, b, kin, kB, idxA, idxB,
                                           (int)cnt, 0, end_bit, s) != hipSuccess)
      return -1;
    std::swap(idxA, idxB);
    return 0;
  };
  auto pass_u64 = [&](const unsigned long long *src, uint64_t cnt) -> int {
    tm_gather(src, idxA, cnt, kA, s);
    return sort_by(kA, cnt, 64);
  };
  auto pass_rank = [&](const uint8_t *src, uint64_t cnt) -> int {
    tm_gather(src, idxA, cnt, kA, s);
    return sort_by(kA, cnt, 1);
  };

  /* ---- 3. candidate cut ---- */
  hipLaunchKernelGGL(k_tm_iota, blocks_of(m), dim3(256), 0, s, idxA, m);
  int rc = sort_by(u0, m, 64);           /* identity order: no gather */
  /* one rank only (no NULL, or nothing but NULL): the u order is final */
  if (!rc && h_seen == 3u) rc = pass_rank(r0, m);
  if (rc) { freeall(); return rc; }
  hipLaunchKernelGGL(k_tm_cut, dim3(1), dim3(64), 0, s, r0, u0, idxA, m, take,
                     d_c);
  unsigned long long h_c = 0;
  e = hipMemcpyAsync(&h_c, d_c, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }
  const uint64_t c = h_c;
  if (c > m || c < (m < take ? m : take)) { freeall(); return -1; }
  *cands = c;

  /* ---- 4. secondary keys, candidates only ---- */
  uint32_t *rows_c = (uint32_t *)dalloc(c * 4);
  /* key 0 of the candidates, in primary order */
  unsigned long long *us = (unsigned long long *)dalloc(c * 8);
  uint8_t *rs = (uint8_t *)dalloc(c);
  unsigned long long *uk[COPR_TOPN_MAX_KEYS] = {us, nullptr, nullptr, nullptr};
  uint8_t *rk[COPR_TOPN_MAX_KEYS] = {rs, nullptr, nullptr, nullptr};
  for (int k = 1; k < n_keys; k++) {
    uk[k] = (unsigned long long *)dalloc(c * 8);
    rk[k] = (uint8_t *)dalloc(c);
  }
  uint32_t *segf = (uint32_t *)dalloc(c * 4);
  uint32_t *seg = (uint32_t *)dalloc(c * 4);
  if (oom) { freeall(); return -2; }
  tm_gather(rows, idxA, c, rows_c, s);
  tm_gather(u0, idxA, c, us, s);
  tm_gather(r0, idxA, c, rs, s);
  /* candidate space from here on: position i = i-th row in primary order */
  hipLaunchKernelGGL(k_tm_iota, blocks_of(c), dim3(256), 0, s, idxA, c);
  if (n_keys > 1) {
    for (int k = 1; k < n_keys; k++)
      if (dev_topn_keys_launch(rgn, rows_c, c, keys[k], uk[k], rk[k], d_err, s)) {
        freeall();
        return -1;
      }
    for (int k = n_keys - 1; k >= 1 && !rc; k--) {
      rc = pass_u64(uk[k], c);
      if (!rc) rc = pass_rank(rk[k], c);
    }
    if (rc) { freeall(); return rc; }
    /* last pass: the primary composite, as its run number */
    hipLaunchKernelGGL(k_tm_seg_flags, blocks_of(c), dim3(256), 0, s, rs, us,
                       c, segf);
    size_t b = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, b, segf, seg, (int)c, s);
    if (!need_tmp(b)) { freeall(); return -2; }
    if (hipcub::DeviceScan::InclusiveSum(tmp, b, segf, seg, (int)c, s) != hipSuccess) {
      freeall();
      return -1;
    }
    int bits = 1;
    while (bits < 32 && (c >> bits)) bits++;      /* run numbers are < c */
    tm_gather(seg, idxA, c, kA, s);
    rc = sort_by(kA, c, bits);
    if (rc) { freeall(); return rc; }
  }

  /* ---- winners ---- */
  const uint64_t tk = c < take ? c : take;
  uint32_t *w_rows = (uint32_t *)dalloc(tk * 4);
  unsigned long long *w_u = (unsigned long long *)dalloc(tk * 8 * n_keys);
  uint8_t *w_r = (uint8_t *)dalloc(tk * n_keys);
  if (oom) { freeall(); return -2; }
  tm_gather(rows_c, idxA, tk, w_rows, s);
  for (int k = 0; k < n_keys; k++) {
    tm_gather(uk[k], idxA, tk, w_u + (uint64_t)k * tk, s);
    tm_gather(rk[k], idxA, tk, w_r + (uint64_t)k * tk, s);
  }
  winners->resize(tk);
  std::vector<unsigned long long> h_u(tk * n_keys);
  std::vector<uint8_t> h_r(tk * n_keys);
  e = hipMemcpyAsync(winners->data(), w_rows, tk * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_u.data(), w_u, tk * 8 * n_keys, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_r.data(), w_r, tk * n_keys, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) { winners->clear(); return -1; }
  if (h_err) { winners->clear(); return -3; }
  for (int k = 0; k < n_keys; k++) {
    key_vals[k].resize(tk);
    key_nulls[k].resize(tk);
    for (uint64_t i = 0; i < tk; i++) {
      int64_t v;
      bool nul;
      topn_key_decode(h_r[(uint64_t)k * tk + i], h_u[(uint64_t)k * tk + i],
                      keys[k].uns != 0, keys[k].desc != 0, &v, &nul);
      key_vals[k][i] = v;
      key_nulls[k][i] = nul ? 1 : 0;
    }
  }
  return 0;
}

}  // namespace copr
