/* topn_keys.h — order-key transform and candidate-cut rule of the multi-key
 * TopN pipeline. Pure C++: no HIP header, no other project
 * header. The device kernels and the host include this file, and so does the
 * stand-alone CPU test, so the tested code is the shipped code. */
#ifndef COPR_TOPN_KEYS_H
#define COPR_TOPN_KEYS_H

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define COPR_TOPN_HD __attribute__((host)) __attribute__((device))
#else
#define COPR_TOPN_HD
#endif

namespace copr {

#define COPR_TOPN_MAX_KEYS 4

/* One order key of one row as (rank, u): ascending order on (rank, u) is the
 * reference comparator for that key (top_n_executor.rs): NULL before every
 * value, values in signed or unsigned order, desc reversing both. rank is one
 * bit. NULL rows carry u = 0 so that all NULLs of a key compare equal. */
COPR_TOPN_HD inline void topn_key_encode(int64_t v, bool is_null, bool uns,
                                         bool desc, uint8_t *rank,
                                         unsigned long long *u) {
  if (is_null) {
    *rank = desc ? 1 : 0;
    *u = 0;
    return;
  }
  unsigned long long x =
      (unsigned long long)v ^ (uns ? 0ull : 0x8000000000000000ull);
  *rank = desc ? 0 : 1;
  *u = desc ? ~x : x;
}

/* inverse: the value and NULL flag a (rank, u) pair was made from */
COPR_TOPN_HD inline void topn_key_decode(uint8_t rank, unsigned long long u,
                                         bool uns, bool desc, int64_t *v,
                                         bool *is_null) {
  *is_null = rank == (desc ? 1 : 0);
  unsigned long long x = desc ? ~u : u;
  *v = *is_null ? 0
                : (int64_t)(x ^ (uns ? 0ull : 0x8000000000000000ull));
}

/* (ra, ua) <= (rb, ub) */
COPR_TOPN_HD inline bool topn_comp_le(uint8_t ra, unsigned long long ua,
                                      uint8_t rb, unsigned long long ub) {
  return ra != rb ? ra < rb : ua <= ub;
}

/* Candidate cut. rank/u hold the primary key's composites of the m kept
 * rows; position i of their ascending order is element perm[i] (perm null:
 * the arrays are in that order themselves). Only the first take =
 * min(n, limit) rows of the final order are emitted. Every row that can be
 * among them has a primary composite <= the one at position take - 1,
 * whatever its other keys are, so the candidate count c is the number of
 * composites <= that cutoff: take <= c <= m, and c = m when m <= take.
 * Binary search (upper bound). */
COPR_TOPN_HD inline uint64_t topn_cut(const uint8_t *rank,
                                      const unsigned long long *u,
                                      const uint32_t *perm, uint64_t m,
                                      uint64_t take) {
  if (take == 0) return 0;
  if (m <= take) return m;
  const uint64_t ic = perm ? perm[take - 1] : take - 1;
  const uint8_t rc = rank[ic];
  const unsigned long long uc = u[ic];
  uint64_t lo = take, hi = m;   /* first position whose composite > cutoff */
  while (lo < hi) {
    uint64_t mid = lo + (hi - lo) / 2;
    uint64_t im = perm ? perm[mid] : mid;
    if (topn_comp_le(rank[im], u[im], rc, uc)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

/* one order key of a multi-key TopN request */
struct TopnKey {
  int64_t col_id;
  int32_t uns;            /* column UNSIGNED flag */
  int32_t desc;
  int32_t missing_null;   /* absent cell: NULL, else missing_val */
  int32_t col_off;        /* scan-column offset (host bookkeeping) */
  int64_t missing_val;
};

}  // namespace copr

#endif
