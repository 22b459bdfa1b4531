/* in_set.h — the set image of an int IN-list predicate: built
 * once per request on the host, probed by the host fold and by both device
 * sites (the RPN evaluator's kind-5 node and k_plane_in). Pure C++: no HIP,
 * no other project header, so build and probe compile and test on their own.
 *
 * Semantics (TiKV compare_in_int_type_by_hash, TiDB builtinInIntSig): the
 * probe equals an item when both denote the same integer, the probe read
 * under the column's UNSIGNED flag and the item under its kind. The image
 * therefore keeps only the items some probe value can equal, as 64-bit
 * patterns: among those, integer equality is pattern equality. */
#ifndef COPR_IN_SET_H
#define COPR_IN_SET_H

#include <stdint.h>
#include <algorithm>
#include <vector>

namespace copr {

#define COPR_IN_MAX_ITEMS 1024
#define COPR_IN_MIN_SLOTS 16u
#define COPR_IN_MAX_SLOTS 2048u

#if defined(__HIP__) || defined(__HIPCC__)
#define COPR_IN_HD __attribute__((host)) __attribute__((device))
#else
#define COPR_IN_HD
#endif

/* one list item as the request states it */
struct InItem {
  uint64_t bits;       /* the i64 / u64 payload */
  uint8_t uns;         /* CONST_UINT */
  uint8_t null;        /* CONST_NULL */
};

/* open-addressed table of tab.size() = mask + 1 slots, linear probing; a free
   slot holds `empty`, which is no key */
struct InSet {
  std::vector<uint64_t> tab;
  uint32_t mask = 0;
  uint64_t empty = 0;
  uint32_t n_keys = 0;
  bool has_null = false;
};

/* multiplicative hash; the product's bits 40..50 index up to 2048 slots */
COPR_IN_HD inline uint32_t in_set_hash(uint64_t v, uint32_t mask) {
  return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> 40) & mask;
}

/* Is v a key? `empty` is tested first, so a probe value that equals it walks
   to the first free slot and misses. At most half the slots are taken, so the
   walk ends; the bound keeps a damaged image from spinning a wave. */
COPR_IN_HD inline bool in_set_probe(const uint64_t *tab, uint32_t mask,
                                    uint64_t empty, uint64_t v) {
  uint32_t i = in_set_hash(v, mask);
  for (uint32_t k = 0; k <= mask; k++) {
    const uint64_t s = tab[i];
    if (s == empty) return false;
    if (s == v) return true;
    i = (i + 1) & mask;
  }
  return false;
}

/* items -> image. Dropped: a negative signed item under an unsigned probe and
   an unsigned item >= 2^63 under a signed probe (no probe value equals them),
   and duplicates. Slots = the power of two >= 2 x keys within [16, 2048].
   empty = the smallest of 0, 1, 2, ... that is no key: with at most 1024 keys
   one of the first 1025 is free. n must not exceed COPR_IN_MAX_ITEMS. */
inline InSet in_set_build(const InItem *items, size_t n, bool probe_unsigned) {
  InSet s;
  std::vector<uint64_t> keys;
  keys.reserve(n);
  for (size_t i = 0; i < n; i++) {
    const InItem &it = items[i];
    if (it.null) { s.has_null = true; continue; }
    if ((it.uns != 0) != probe_unsigned && (it.bits >> 63)) continue;
    keys.push_back(it.bits);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  s.n_keys = (uint32_t)keys.size();
  uint32_t slots = COPR_IN_MIN_SLOTS;
  while (slots < 2u * s.n_keys && slots < COPR_IN_MAX_SLOTS) slots <<= 1;
  s.mask = slots - 1;
  /* keys are sorted: the first gap in 0, 1, 2, ... */
  uint64_t e = 0;
  for (uint64_t k : keys) {
    if (k != e) break;
    e++;
  }
  s.empty = e;
  s.tab.assign(slots, e);
  for (uint64_t k : keys) {
    uint32_t i = in_set_hash(k, s.mask);
    while (s.tab[i] != e) i = (i + 1) & s.mask;
    s.tab[i] = k;
  }
  return s;
}

/* the node's three-valued result on a non-NULL probe, as the host fold and
   the reference of the CPU test read it: 1 true, 0 false, -1 NULL */
inline int in_set_eval(const InSet &s, uint64_t v) {
  if (in_set_probe(s.tab.data(), s.mask, s.empty, v)) return 1;
  return s.has_null ? -1 : 0;
}

/* what the plane kernels take per request (k_plane_in, k_plane_inb): keep =
   (probe hit) != invert for an int row; never = NOT IN over a list with a
   NULL, which keeps no row; keep_absent = the same test on the column's
   default fill (0 when that is NULL). */
struct InFcArgs {
  uint32_t invert, never, keep_absent;
};

inline void in_fc_fold(const InSet &s, bool negate, bool missing_null,
                       int64_t missing_val, InFcArgs *fa) {
  fa->invert = negate ? 1u : 0u;
  fa->never = (negate && s.has_null) ? 1u : 0u;
  const bool hit = !missing_null &&
                   in_set_probe(s.tab.data(), s.mask, s.empty,
                                (uint64_t)missing_val);
  fa->keep_absent = (!missing_null && !fa->never && hit != negate) ? 1u : 0u;
}

/* ---- the list over a split 32-bit plane (k_plane_ins) --------
 * The plane stores n = v - base in [0, nmax], nmax < 2^32, as h = n >> 16 and
 * l = n & 0xFFFF. A key k is a value of the plane exactly when d = k - base,
 * taken modulo 2^64 over the patterns as in k_plane_inb, is <= nmax (base +
 * nmax does not wrap, for either signedness); its bucket is d >> 16. A row
 * whose h names no flagged bucket cannot hit, whatever its l. */
COPR_IN_HD inline bool in_split_bucket(uint64_t k, uint64_t empty,
                                       uint64_t base, uint64_t nmax,
                                       uint32_t *bucket) {
  const uint64_t d = k - base;
  if (k == empty || d > nmax || d > 0xFFFFFFFFull) return false;
  *bucket = (uint32_t)(d >> 16);
  return true;
}

/* the hull [hull_lo, hull_lo + hull_span] of the flagged buckets, also in the
   packed 16-bit form of DESIGN §9l (the value in both halves of a word, for
   packed_out_acc); none = no key lies in the plane's domain, the hull is then
   unused (zero). flagged = how many buckets hold a key, of buckets = (nmax >>
   16) + 1: the share of a uniform plane's rows that reach the probe. */
struct InSplitArgs {
  uint32_t hull_lo, hull_span;
  uint32_t hull_lo_pk, hull_span_pk;
  uint32_t none;
  uint32_t flagged, buckets;
};

/* image + plane domain -> InSplitArgs and, when bm is given, the bucket bitmap
   the kernel builds in LDS: (nmax >> 21) + 1 words */
inline void in_split_fold(const InSet &s, int64_t base, uint64_t nmax,
                          InSplitArgs *a, std::vector<uint32_t> *bm = nullptr) {
  uint32_t lo = 0xFFFFFFFFu, hi = 0;
  std::vector<uint32_t> own;
  if (!bm) bm = &own;
  bm->assign((size_t)(nmax >> 21) + 1, 0u);
  a->flagged = 0;
  a->buckets = (uint32_t)(nmax >> 16) + 1u;
  for (uint64_t k : s.tab) {
    uint32_t b;
    if (!in_split_bucket(k, s.empty, (uint64_t)base, nmax, &b)) continue;
    lo = b < lo ? b : lo;
    hi = b > hi ? b : hi;
    if (!(((*bm)[b >> 5] >> (b & 31u)) & 1u)) a->flagged++;
    (*bm)[b >> 5] |= 1u << (b & 31u);
  }
  a->none = lo > hi ? 1u : 0u;
  a->hull_lo = a->none ? 0u : lo;
  a->hull_span = a->none ? 0u : hi - lo;
  a->hull_lo_pk = a->hull_lo * 0x10001u;
  a->hull_span_pk = a->hull_span * 0x10001u;
}

/* the row rule: a clear bucket bit misses; a set one probes the image with
   the row's full value; keep = hit != invert, and never keeps nothing. h must
   not exceed nmax >> 16 (every row of the plane obeys). */
COPR_IN_HD inline bool in_split_row(uint32_t h, uint32_t l, const uint32_t *bm,
                                    const uint64_t *tab, uint32_t mask,
                                    uint64_t empty, uint64_t base,
                                    uint32_t invert, uint32_t never) {
  if (never) return false;
  bool hit = false;
  if ((bm[h >> 5] >> (h & 31u)) & 1u)
    hit = in_set_probe(tab, mask, empty, base + (((uint64_t)h << 16) | l));
  return hit != (invert != 0);
}

}  // namespace copr
#endif
