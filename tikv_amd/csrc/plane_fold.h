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

/* a AND b over one column: both from plane_fc_fold with the same
   signedness, so the keys share bias. true = *out is the one interval test
   that keeps exactly the values both keep; false = the conjunction is not one
   interval (an NE point strictly inside an interval, two different NE
   points) and the request stays where it was. An inverted test is "never"
   (the whole range) or an NE point; any other inverted form is refused. */
inline bool plane_fc_and(const PlaneFcArgs &a, const PlaneFcArgs &b,
                         PlaneFcArgs *out) {
  const unsigned long long MAXU = ~0ull;
  if (a.bias != b.bias) return false;
  auto never = [&](const PlaneFcArgs &x) {
    return x.invert && x.lo == 0 && x.span == MAXU;
  };
  out->bias = a.bias;
  out->invert = 0;
  out->keep_absent = (a.keep_absent && b.keep_absent) ? 1u : 0u;
  if (never(a) || never(b)) {
    out->lo = 0; out->span = MAXU; out->invert = 1; out->keep_absent = 0;
    return true;
  }
  if ((a.invert && a.span) || (b.invert && b.span)) return false;
  if (a.invert && b.invert) {                       /* two NE points */
    if (a.lo != b.lo) return false;
    out->lo = a.lo; out->span = 0; out->invert = 1;
    return true;
  }
  unsigned long long lo, hi;
  if (!a.invert && !b.invert) {                     /* two intervals */
    const unsigned long long ha = a.lo + a.span, hb = b.lo + b.span;
    lo = a.lo > b.lo ? a.lo : b.lo;
    hi = ha < hb ? ha : hb;
  } else {                                          /* interval, NE point */
    const PlaneFcArgs &iv = a.invert ? b : a;
    const unsigned long long p = a.invert ? a.lo : b.lo;
    lo = iv.lo;
    hi = iv.lo + iv.span;
    if (p > lo && p < hi) return false;
    if (p == lo && p == hi) { lo = 1; hi = 0; }     /* nothing left */
    else if (p == lo) lo++;
    else if (p == hi) hi--;
  }
  if (lo > hi) {
    out->lo = 0; out->span = MAXU; out->invert = 1; out->keep_absent = 0;
    return true;
  }
  out->lo = lo;
  out->span = hi - lo;
  return true;
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
   {0x10000, 0}, false for every h <= 0xFFFF.
   The *_pk fields are the same intervals for the packed count,
   the 16-bit value in both halves of a word. The empty sure interval has no
   16-bit form: sure_empty says so and sure_*_pk are then unused (zero). */
struct SplitFcArgs {
  uint32_t lo, span, invert;       /* the full test, as NarrowFcArgs */
  uint32_t maybe_lo, maybe_span;
  uint32_t sure_lo, sure_span;
  uint32_t maybe_lo_pk, maybe_span_pk;
  uint32_t sure_lo_pk, sure_span_pk;
  uint32_t sure_empty;
};

#if defined(__HIP__) || defined(__HIPCC__)
#define COPR_FOLD_HD __attribute__((host)) __attribute__((device))
#else
#define COPR_FOLD_HD
#endif

/* x (<= 0xFFFF, larger values saturate) in both 16-bit halves of a word */
COPR_FOLD_HD inline uint32_t fold_pack16(uint32_t x) {
  return (x > 0xFFFFu ? 0xFFFFu : x) * 0x10001u;
}

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
  sf->maybe_lo_pk = fold_pack16(sf->maybe_lo);
  sf->maybe_span_pk = fold_pack16(sf->maybe_span);
  sf->sure_empty = sf->sure_lo > 0xFFFFu ? 1u : 0u;
  sf->sure_lo_pk = sf->sure_empty ? 0u : fold_pack16(sf->sure_lo);
  sf->sure_span_pk = sf->sure_empty ? 0u : fold_pack16(sf->sure_span);
}

/* The packed count: how many of the two 16-bit halves of w lie
   outside [lo, lo + span], lo and span the same 16-bit value in both halves
   of lo_pk and span_pk and lo + span <= 0xFFFF. Four steps, each one packed
   16-bit instruction on the device (narrow_planes.hip, packed_out_acc):
     d = w - lo        per half, wrapping      (a half below lo wraps high)
     e = d - span      per half, clamped at 0  (0 exactly when d <= span)
     m = min(e, 1)     per half
     count = m.lo + m.hi
   This is the arithmetic the device code is meant to perform, one word at a
   time and summed at once; the device helper takes a 16 B vector, keeps the
   two counts packed in its accumulator and sums the halves once per
   iteration (packed_sum). The CPU test checks this arithmetic against the
   per-row tests. That the inline assembly performs it (clamp semantics,
   operand order) is checked by the GPU tests alone (test_packed_fc.py). */
COPR_FOLD_HD inline uint32_t fold_pk_sub_u16(uint32_t a, uint32_t b) {
  return ((a - (b & 0xFFFFu)) & 0xFFFFu) |
         ((a - (b & 0xFFFF0000u)) & 0xFFFF0000u);
}
COPR_FOLD_HD inline uint32_t fold_pk_sub_sat_u16(uint32_t a, uint32_t b) {
  const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu;
  const uint32_t ah = a >> 16, bh = b >> 16;
  return (al > bl ? al - bl : 0u) | ((ah > bh ? ah - bh : 0u) << 16);
}
COPR_FOLD_HD inline uint32_t fold_pk_min_u16(uint32_t a, uint32_t b) {
  const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu;
  const uint32_t ah = a >> 16, bh = b >> 16;
  return (al < bl ? al : bl) | ((ah < bh ? ah : bh) << 16);
}
COPR_FOLD_HD inline uint32_t fold_packed_out(uint32_t w, uint32_t lo_pk,
                                             uint32_t span_pk) {
  const uint32_t d = fold_pk_sub_u16(w, lo_pk);
  const uint32_t e = fold_pk_sub_sat_u16(d, span_pk);
  const uint32_t m = fold_pk_min_u16(e, 0x00010001u);
  return (m & 0xFFFFu) + (m >> 16);
}

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

/* k_plane_fcb: a split plane's bucket index holds the low halves
   grouped by h and off[0 .. 65536], bucket h at [off[h], off[h + 1]). The rows
   of the sure interval are counted by two offsets; a maybe bucket that is not
   sure, the one holding a >> 16 and the one holding b >> 16, is a slice
   [beg, end) of the grouped low halves whose rows take split_full_in(h, l).
   n_slices = 1 when a >> 16 == b >> 16, 0 when both edge buckets are sure; a
   slice may be empty. in = sure + the slices' rows that pass, and
   count = invert ? n_rows - in : in. */
#define COPR_N_BUCKETS 65536u
struct BucketFcArgs {
  uint64_t sure;                   /* rows in the sure interval */
  uint64_t beg[2], end[2];         /* beg <= end <= n_rows */
  uint32_t h[2];
  uint32_t n_slices;
  uint32_t invert;
};

/* SplitFcArgs (not the all_lo form) + offsets -> BucketFcArgs. off must be
   non-decreasing with off[65536] == n_rows; false = it is not, at the entries
   this request reads, and the request keeps the scan. */
inline bool bucket_fc_fold(const SplitFcArgs &sf, const uint64_t *off,
                           uint64_t n_rows, BucketFcArgs *ba) {
  *ba = BucketFcArgs{};
  ba->invert = sf.invert;
  if (!sf.sure_empty) {
    const uint64_t s0 = off[sf.sure_lo], s1 = off[sf.sure_lo + sf.sure_span + 1];
    if (s0 > s1 || s1 > n_rows) return false;
    ba->sure = s1 - s0;
  }
  const uint32_t ha = sf.maybe_lo, hb = sf.maybe_lo + sf.maybe_span;
  const uint32_t edge[2] = {ha, hb};
  for (int i = 0; i < (ha == hb ? 1 : 2); i++) {
    const uint32_t h = edge[i];
    if (h >= COPR_N_BUCKETS) return false;
    if (split_sure(h, sf)) continue;
    const uint64_t b = off[h], e = off[h + 1];
    if (b > e || e > n_rows) return false;
    ba->h[ba->n_slices] = h;
    ba->beg[ba->n_slices] = b;
    ba->end[ba->n_slices] = e;
    ba->n_slices++;
  }
  return true;
}

}  // namespace copr
#endif
