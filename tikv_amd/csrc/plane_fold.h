/* plane_fold.h — host folds of a cmp(col, const) filter into the range tests
 * of the filter+count plane kernels. Pure C++: no HIP, no
 * other project header, so the folds compile and test on their own. */
#ifndef COPR_PLANE_FOLD_H
#define COPR_PLANE_FOLD_H

#include <stdint.h>

namespace copr {

/* compare kinds (order matches oracle CmpKind) */
enum { CMP_LT = 0, CMP_LE, CMP_GT, CMP_GE, CMP_EQ, CMP_NE };

/* k_plane_fc: keep = (((v ^ bias) - lo) <= span) != invert over the full
   64-bit value; keep_absent = what an ABSENT row does under the request's
   default fill. */
struct PlaneFcArgs {
  unsigned long long bias, lo, span;
  uint32_t invert, keep_absent;
};

/* comparer, signedness and constant -> PlaneFcArgs. [lo, lo + span] never
   wraps. A NULL constant and a comparer no value can satisfy come out as
   "never" = the whole range, inverted. */
inline void plane_fc_fold(int cmp, int64_t cst, bool uns, bool const_null,
                          bool missing_null, int64_t missing_val,
                          PlaneFcArgs *fa) {
  const unsigned long long MAXU = ~0ull;
  fa->bias = uns ? 0ull : 0x8000000000000000ull;
  const unsigned long long c = (unsigned long long)cst ^ fa->bias;
  bool empty = false;
  fa->invert = 0;
  switch (cmp) {
    case CMP_LT: empty = c == 0; fa->lo = 0; fa->span = c - 1; break;
    case CMP_LE: fa->lo = 0; fa->span = c; break;
    case CMP_GT: empty = c == MAXU; fa->lo = c + 1; fa->span = MAXU - (c + 1); break;
    case CMP_GE: fa->lo = c; fa->span = MAXU - c; break;
    case CMP_EQ: fa->lo = c; fa->span = 0; break;
    default:     fa->lo = c; fa->span = 0; fa->invert = 1; break;   /* NE */
  }
  if (empty || const_null) {   /* never true: all-range, inverted */
    fa->lo = 0; fa->span = MAXU; fa->invert = 1;
  }
  unsigned long long mk = (unsigned long long)missing_val ^ fa->bias;
  fa->keep_absent = (!missing_null &&
                     (((mk - fa->lo) <= fa->span) != (fa->invert != 0)))
                        ? 1u : 0u;
}

/* k_plane_fcn: keep = ((n - lo) <= span) != invert in 32-bit unsigned
   arithmetic over the narrow plane's n = (uint)(v - base). */
struct NarrowFcArgs {
  uint32_t lo, span, invert;
};

/* PlaneFcArgs -> the narrow domain of a plane whose every row is an int in
   [base, base + nmax] (signed; nmax < 2^32). The key of a stored n is
   n + key(base), so the request's closed key interval is cut down to the
   plane's and shifted by key(base); an empty cut keeps no row (every row
   under invert). uns = the request reads the column as unsigned: signed and
   unsigned order agree on the plane only when base and base + nmax have the
   same sign, otherwise false = the request cannot use the narrow plane.
   keep_absent plays no part: a narrow plane has no ABSENT row. */
inline bool narrow_fc_fold(const PlaneFcArgs &fa, int64_t base, uint64_t nmax,
                           bool uns, NarrowFcArgs *nf) {
  if (nmax > 0xFFFFFFFFull) return false;
  /* base + nmax <= INT64_MAX by construction, so the sum does not wrap */
  const int64_t top = (int64_t)((uint64_t)base + nmax);
  if (uns && (base < 0) != (top < 0)) return false;
  const unsigned long long kb = (unsigned long long)base ^ fa.bias;
  const unsigned long long kt = kb + nmax;
  const unsigned long long hi = fa.lo + fa.span;
  const unsigned long long a = fa.lo > kb ? fa.lo : kb;
  const unsigned long long b = hi < kt ? hi : kt;
  nf->invert = fa.invert ? 1u : 0u;
  if (a > b) {            /* no stored value inside the request's interval */
    nf->lo = 0; nf->span = 0xFFFFFFFFu; nf->invert ^= 1u;
    return true;
  }
  nf->lo = (uint32_t)(a - kb);
  nf->span = (uint32_t)(b - a);
  return true;
}

/* k_plane_fcs: a 4-byte narrow plane is stored as two 16-bit
   planes, h = n >> 16 and l = n & 0xFFFF, and the kernel streams h alone.
   With the narrow test a <= n <= b (a = lo, b = lo + span):
     maybe = h in [a >> 16, b >> 16]; a row outside it fails the test;
     sure  = maybe shrunk to the h whose every l passes the test;
   only a row in maybe and not in sure needs its l. Both are range tests in
   32-bit unsigned arithmetic, (h - x_lo) <= x_span; an empty sure interval is
   {0x10000, 0}, false for every h <= 0xFFFF. */
struct SplitFcArgs {
  uint32_t lo, span, invert;       /* the full test, as NarrowFcArgs */
  uint32_t maybe_lo, maybe_span;
  uint32_t sure_lo, sure_span;
};

/* NarrowFcArgs -> SplitFcArgs. [lo, lo + span] does not wrap (narrow_fc_fold
   guarantees it), so its "never" form, the whole range inverted, comes out as
   sure = every h. all_lo = the measuring switch COPR_SPLIT_ALL_LO: maybe =
   every h, sure = empty, so every row is resolved from both halves. */
inline void split_fc_fold(const NarrowFcArgs &nf, bool all_lo,
                          SplitFcArgs *sf) {
  sf->lo = nf.lo;
  sf->span = nf.span;
  sf->invert = nf.invert;
  const uint32_t a = nf.lo, b = nf.lo + nf.span;
  sf->maybe_lo = a >> 16;
  sf->maybe_span = (b >> 16) - (a >> 16);
  const int64_t s_lo = (int64_t)(a >> 16) + ((a & 0xFFFFu) != 0 ? 1 : 0);
  const int64_t s_hi = (int64_t)(b >> 16) - ((b & 0xFFFFu) != 0xFFFFu ? 1 : 0);
  if (all_lo) {
    sf->maybe_lo = 0;
    sf->maybe_span = 0xFFFFu;
  }
  if (all_lo || s_lo > s_hi) {
    sf->sure_lo = 0x10000u;
    sf->sure_span = 0;
  } else {
    sf->sure_lo = (uint32_t)s_lo;
    sf->sure_span = (uint32_t)(s_hi - s_lo);
  }
}

#if defined(__HIP__) || defined(__HIPCC__)
#define COPR_FOLD_HD __attribute__((host)) __attribute__((device))
#else
#define COPR_FOLD_HD
#endif

/* the row rule of a split plane, before invert: keep = in != invert.
   k_plane_fcs applies the three steps in two phases, the first two to every
   row and split_full_in to the rows they leave open. */
COPR_FOLD_HD inline bool split_maybe(uint32_t h, const SplitFcArgs &sf) {
  return (h - sf.maybe_lo) <= sf.maybe_span;
}
COPR_FOLD_HD inline bool split_sure(uint32_t h, const SplitFcArgs &sf) {
  return (h - sf.sure_lo) <= sf.sure_span;
}
COPR_FOLD_HD inline bool split_full_in(uint32_t h, uint32_t l,
                                       const SplitFcArgs &sf) {
  return (((h << 16) | l) - sf.lo) <= sf.span;
}
COPR_FOLD_HD inline bool split_row_in(uint32_t h, uint32_t l,
                                      const SplitFcArgs &sf) {
  if (!split_maybe(h, sf)) return false;
  if (split_sure(h, sf)) return true;
  return split_full_in(h, l, sf);
}

}  // namespace copr
#endif
