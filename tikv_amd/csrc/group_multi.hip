/* group_multi.hip — stage 1 of hash aggregation over several int group-by
 * columns: every row's tuple of key cells -> one exact group id.
 *
 * The dictionary is a power-of-two array of 64-bit slot words (group_keys.h):
 * 0 = empty, else (fingerprint << 32) | (representative row + 1). A slot is
 * claimed with one atomicCAS from 0 and never changes afterwards; a prober
 * that meets its own fingerprint reads the representative row's cells from the
 * kernel's immutable inputs and compares the tuples exactly. Nothing is
 * published after the claim, nothing waits on another lane, and no key value
 * is a sentinel. gid[row] = the slot index, written for every row of the
 * region (the filters run in stage 2), in a buffer shaped like a column plane
 * so that k_plane_hash takes it as its group plane.
 * The row-bytes key source needs the row parsers: dev_topn_keys_launch in
 * kernels.hip. */
#include <hip/hip_runtime.h>
#include "copr_internal.h"

namespace copr {

/* one key's cell of one row; false = a plane state stage 1 does not serve */
__device__ static inline bool gk_cell(const GkSrc &s, uint64_t row, int64_t *v,
                                      uint8_t *nul) {
  if (s.kind == 0) {
    switch (s.st[row]) {
      case PST_INT: *v = s.val[row]; *nul = 0; return true;
      case PST_NULL: *v = 0; *nul = 1; return true;
      case PST_ABSENT:
        *nul = s.missing_null ? 1 : 0;
        *v = s.missing_null ? 0 : s.missing_val;
        return true;
      default: *v = 0; *nul = 1; return false;
    }
  }
  bool is_null;
  topn_key_decode(s.st[row], (unsigned long long)s.val[row], s.uns != 0, false,
                  v, &is_null);
  *nul = is_null ? 1 : 0;
  return true;
}

__device__ static inline bool gk_tuple(const GkArgs &a, uint64_t row,
                                       GkTuple *t) {
  bool ok = true;
  #pragma unroll
  for (int k = 0; k < COPR_GROUP_MAX_KEYS; k++) {
    t->v[k] = 0;
    t->nul[k] = 0;
    if (k < a.n_keys) ok &= gk_cell(a.k[k], row, &t->v[k], &t->nul[k]);
  }
  return ok;
}

/* flags[0] = dictionary full, flags[1] = a plane row outside INT / NULL /
 * ABSENT (the host reruns on the row-bytes source) */
__global__ void __launch_bounds__(256)
k_gk_dict(GkArgs a, uint64_t n_rows, unsigned long long *__restrict__ slots,
          uint32_t mask, int64_t *__restrict__ gid,
          unsigned int *__restrict__ flags,
          unsigned long long *__restrict__ n_filled) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool full = false, fallback = false;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < n_rows; row += stride) {
    GkTuple t;
    if (!gk_tuple(a, row, &t)) {
      fallback = true;
      gid[row] = 0;
      continue;
    }
    bool claimed;
    int64_t slot = gk_probe(
        t, a.n_keys, row, mask,
        [&](uint32_t s) -> uint64_t {
          return __hip_atomic_load(&slots[s], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        },
        [&](uint32_t s, uint64_t w) -> uint64_t {
          return atomicCAS(&slots[s], 0ull, (unsigned long long)w);
        },
        [&](uint64_t rep) -> GkTuple {
          GkTuple o;
          /* rep < n_rows: only rows of this launch claim slots. Its states
             were accepted by the lane that claimed; a lane that has not got
             there yet still reads the same immutable cells. */
          gk_tuple(a, rep < n_rows ? rep : row, &o);
          return o;
        },
        &claimed);
    if (claimed) atomicAdd(n_filled, 1ull);
    if (slot < 0) full = true;
    gid[row] = slot < 0 ? 0 : slot;
  }
  if (full) atomicOr(flags, 1u);
  if (fallback) atomicOr(flags + 1, 1u);
}

/* slot -> representative row -> the K (value, NULL) cells, key-major */
__global__ void __launch_bounds__(256)
k_gk_gather(GkArgs a, uint64_t n_rows,
            const unsigned long long *__restrict__ slots, uint32_t mask,
            const uint32_t *__restrict__ which, uint64_t cnt,
            int64_t *__restrict__ out_v, uint8_t *__restrict__ out_n,
            unsigned int *__restrict__ flags) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t s = which[i];
  const uint64_t w = s <= mask ? slots[s] : 0;
  GkTuple t{};
  if (w == 0 || gk_slot_row(w) >= n_rows) atomicOr(flags, 1u);
  else gk_tuple(a, gk_slot_row(w), &t);
  #pragma unroll
  for (int k = 0; k < COPR_GROUP_MAX_KEYS; k++) {
    if (k >= a.n_keys) break;
    out_v[(uint64_t)k * cnt + i] = t.v[k];
    out_n[(uint64_t)k * cnt + i] = t.nul[k];
  }
}

__global__ void __launch_bounds__(256)
k_gk_iota(uint32_t *__restrict__ idx, uint64_t cnt) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) idx[i] = (uint32_t)i;
}

void dev_group_free(GroupIds *g) {
  (void)hipFree(g->gid_val);
  (void)hipFree(g->gid_st);
  (void)hipFree(g->slots);
  (void)hipFree(g->d_flags);
  for (int k = 0; k < COPR_GROUP_MAX_KEYS; k++) {
    (void)hipFree(g->row_u[k]);
    (void)hipFree(g->row_rank[k]);
  }
  /* the run counters outlive the buffers: a failed stage still reports them */
  GroupIds z{};
  z.grows = g->grows;
  z.row_source_runs = g->row_source_runs;
  *g = z;
}

int dev_group_ids(const DevRegion &rgn, const GroupKey *keys, int n_keys,
                  const PlaneRef *planes, uint32_t init_slots, void *stream,
                  GroupIds *g) {
  hipStream_t s = (hipStream_t)stream;
  const uint64_t n = rgn.n_kv;
  *g = GroupIds{};
  if (n_keys < 1 || n_keys > COPR_GROUP_MAX_KEYS || n >= 0xFFFFFFFFull ||
      !init_slots || (init_slots & (init_slots - 1)))
    return -1;
  g->n_rows = n;
  g->args.n_keys = n_keys;
  if (!n) return 0;

  /* the gid buffer: a column plane of PST_INT rows, same tail slack */
  hipError_t e = hipMalloc((void **)&g->gid_val, n * 8 + 2048);
  if (e == hipSuccess) e = hipMalloc((void **)&g->gid_st, n + 2048);
  if (e == hipSuccess) e = hipMalloc((void **)&g->d_flags, 16);
  if (e != hipSuccess) { dev_group_free(g); return -2; }
  e = hipMemsetAsync(g->gid_st, PST_INT, n + 2048, s);
  if (e != hipSuccess) { dev_group_free(g); return -1; }
  unsigned long long *d_filled = (unsigned long long *)(g->d_flags + 2);

  bool all_rows = false;       /* every key from the row bytes */
  for (;;) {
    /* key sources */
    bool any_row = false;
    for (int k = 0; k < n_keys; k++) {
      GkSrc &src = g->args.k[k];
      src.uns = keys[k].uns;
      src.missing_null = keys[k].missing_null;
      src.missing_val = keys[k].missing_val;
      if (!all_rows && planes && planes[k].val) {
        src.kind = 0;
        src.val = planes[k].val;
        src.st = planes[k].st;
        continue;
      }
      any_row = true;
      if (!g->row_u[k]) {
        e = hipMalloc((void **)&g->row_u[k], n * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&g->row_rank[k], n);
        if (e != hipSuccess) { dev_group_free(g); return -2; }
      }
      src.kind = 1;
      src.val = (const int64_t *)g->row_u[k];
      src.st = g->row_rank[k];
    }
    e = hipMemsetAsync(g->d_flags, 0, 16, s);
    if (e != hipSuccess) { dev_group_free(g); return -1; }
    if (any_row) {
      g->row_source_runs++;
      uint32_t *d_rows = nullptr;
      if (hipMalloc((void **)&d_rows, n * 4) != hipSuccess) {
        dev_group_free(g);
        return -2;
      }
      hipLaunchKernelGGL(k_gk_iota, dim3((uint32_t)((n + 255) / 256)),
                         dim3(256), 0, s, d_rows, n);
      int rc = 0;
      unsigned int *d_err = g->d_flags + 1;   /* read and cleared below */
      for (int k = 0; k < n_keys && !rc; k++) {
        if (g->args.k[k].kind != 1) continue;
        TopnKey tk{};
        tk.col_id = keys[k].col_id;
        tk.uns = keys[k].uns;
        tk.desc = 0;
        tk.missing_null = keys[k].missing_null;
        tk.missing_val = keys[k].missing_val;
        rc = dev_topn_keys_launch(rgn, d_rows, n, tk, g->row_u[k],
                                  g->row_rank[k], d_err, s);
      }
      unsigned int h_err = 0;
      if (!rc) e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
      if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
      (void)hipFree(d_rows);
      if (rc || e != hipSuccess) { dev_group_free(g); return -1; }
      if (h_err) { dev_group_free(g); return -3; }
      e = hipMemsetAsync(g->d_flags, 0, 16, s);
      if (e != hipSuccess) { dev_group_free(g); return -1; }
    }

    /* dictionary: grow x2 and rerun on full */
    uint32_t n_slots = g->n_slots ? g->n_slots : init_slots;
    bool fallback = false;
    for (;;) {
      if (g->n_slots != n_slots) {
        (void)hipFree(g->slots);
        g->slots = nullptr;
        g->n_slots = 0;
        if (hipMalloc((void **)&g->slots, (size_t)n_slots * 8) != hipSuccess) {
          dev_group_free(g);
          return -2;
        }
        g->n_slots = n_slots;
      }
      e = hipMemsetAsync(g->slots, 0, (size_t)n_slots * 8, s);
      if (e == hipSuccess) e = hipMemsetAsync(g->d_flags, 0, 16, s);
      if (e != hipSuccess) { dev_group_free(g); return -1; }
      uint32_t grid = (uint32_t)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
      hipLaunchKernelGGL(k_gk_dict, dim3(grid), dim3(256), 0, s, g->args, n,
                         g->slots, n_slots - 1u, g->gid_val, g->d_flags,
                         d_filled);
      e = hipGetLastError();
      unsigned int h_flags[4] = {0, 0, 0, 0};
      if (e == hipSuccess)
        e = hipMemcpyAsync(h_flags, g->d_flags, 16, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) { dev_group_free(g); return -1; }
      if (h_flags[1]) { fallback = true; break; }
      if (h_flags[0]) {
        if (n_slots >= (1u << 31)) { dev_group_free(g); return -2; }
        n_slots <<= 1;
        g->grows++;
        continue;
      }
      unsigned long long filled;
      memcpy(&filled, h_flags + 2, 8);
      g->n_groups = filled;
      break;
    }
    if (!fallback) return 0;
    if (all_rows) { dev_group_free(g); return -1; }   /* cannot happen */
    all_rows = true;
  }
}

int dev_group_gather(const GroupIds &g, const uint32_t *h_slots, uint64_t cnt,
                     void *stream, std::vector<int64_t> *vals,
                     std::vector<uint8_t> *nulls) {
  hipStream_t s = (hipStream_t)stream;
  const int K = g.args.n_keys;
  vals->assign((size_t)K * cnt, 0);
  nulls->assign((size_t)K * cnt, 0);
  if (!cnt) return 0;
  if (!g.slots || !g.n_rows) return -1;
  uint32_t *d_which = nullptr;
  int64_t *d_v = nullptr;
  uint8_t *d_n = nullptr;
  auto freeall = [&]() {
    (void)hipFree(d_which);
    (void)hipFree(d_v);
    (void)hipFree(d_n);
  };
  hipError_t e = hipMalloc((void **)&d_which, cnt * 4);
  if (e == hipSuccess) e = hipMalloc((void **)&d_v, (size_t)K * cnt * 8);
  if (e == hipSuccess) e = hipMalloc((void **)&d_n, (size_t)K * cnt);
  if (e != hipSuccess) { freeall(); return -2; }
  e = hipMemcpyAsync(d_which, h_slots, cnt * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(g.d_flags, 0, 16, s);
  if (e != hipSuccess) { freeall(); return -1; }
  hipLaunchKernelGGL(k_gk_gather, dim3((uint32_t)((cnt + 255) / 256)),
                     dim3(256), 0, s, g.args, g.n_rows, g.slots,
                     g.n_slots - 1u, d_which, cnt, d_v, d_n, g.d_flags);
  e = hipGetLastError();
  unsigned int h_bad = 0;
  if (e == hipSuccess)
    e = hipMemcpyAsync(vals->data(), d_v, (size_t)K * cnt * 8,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(nulls->data(), d_n, (size_t)K * cnt,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_bad, g.d_flags, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  return (e != hipSuccess || h_bad) ? -1 : 0;
}

}  // namespace copr
