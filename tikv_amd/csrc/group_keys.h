/* group_keys.h — tuple dictionary of multi-key hash aggregation:
 * slot word pack / unpack, tuple hash and fingerprint, tuple equality and the
 * probe rule. Pure C++: no HIP header, no other project header. The device
 * kernels and the host include this file, and so does the stand-alone CPU
 * test, so the tested code is the shipped code. */
#ifndef COPR_GROUP_KEYS_H
#define COPR_GROUP_KEYS_H

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define COPR_GK_HD __attribute__((host)) __attribute__((device))
#define COPR_GK_UNROLL _Pragma("unroll")
#else
#define COPR_GK_HD
#define COPR_GK_UNROLL
#endif

namespace copr {

#define COPR_GROUP_MAX_KEYS 4

/* A dictionary slot: 0 = empty, else (fp32 << 32) | (rep_row + 1). rep_row is
 * the first row that claimed the slot; it is < 2^32 - 1, so the low half is
 * never 0 and a filled word is never 0 whatever the fingerprint is. */
COPR_GK_HD inline uint64_t gk_slot_pack(uint32_t fp, uint64_t rep_row) {
  return ((uint64_t)fp << 32) | (uint64_t)(uint32_t)(rep_row + 1);
}
COPR_GK_HD inline uint32_t gk_slot_fp(uint64_t w) { return (uint32_t)(w >> 32); }
COPR_GK_HD inline uint64_t gk_slot_row(uint64_t w) {
  return (uint64_t)(uint32_t)w - 1;
}

/* the single-key hash table's mixer (d_group_hash in kernels.hip) */
COPR_GK_HD inline uint64_t gk_word_hash(uint64_t key) {
  uint64_t h = key * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

/* One tuple of K (value, NULL) cells. A NULL cell carries value 0, so two
 * NULLs of one column agree in both words. */
struct GkTuple {
  int64_t v[COPR_GROUP_MAX_KEYS];
  uint8_t nul[COPR_GROUP_MAX_KEYS];
};

/* hash of the tuple: each cell's value word and NULL word go through
 * gk_word_hash, chained so that (1,2) and (2,1) differ. The slot index comes
 * from the low bits, the fingerprint from the high 32. */
COPR_GK_HD inline uint64_t gk_tuple_hash(const GkTuple &t, int k) {
  uint64_t h = 0x243F6A8885A308D3ull;
  /* fixed trip count: the tuple stays in registers on the device */
  COPR_GK_UNROLL
  for (int i = 0; i < COPR_GROUP_MAX_KEYS; i++) {
    if (i >= k) break;
    uint64_t v = t.nul[i] ? 0ull : (uint64_t)t.v[i];
    h = gk_word_hash(h ^ gk_word_hash(v));
    h = gk_word_hash(h + (t.nul[i] ? 0x9E3779B97F4A7C15ull : 1ull));
  }
  return h;
}
COPR_GK_HD inline uint32_t gk_hash_slot(uint64_t h, uint32_t mask) {
  return (uint32_t)h & mask;
}
COPR_GK_HD inline uint32_t gk_hash_fp(uint64_t h) { return (uint32_t)(h >> 32); }

/* same group: per column both NULL, or both values with the same 64 bits */
COPR_GK_HD inline bool gk_tuple_eq(const GkTuple &a, const GkTuple &b, int k) {
  bool eq = true;
  COPR_GK_UNROLL
  for (int i = 0; i < COPR_GROUP_MAX_KEYS; i++) {
    if (i >= k) break;
    eq &= (a.nul[i] != 0) == (b.nul[i] != 0);
    eq &= a.nul[i] || a.v[i] == b.v[i];
  }
  return eq;
}

/* Find-or-claim t's slot. The caller supplies how a slot is read (load), how
 * an empty one is claimed (cas: returns the word found, 0 = the claim won)
 * and how a representative row's tuple is fetched (tuple_of), so the device
 * kernel (atomics, plane loads) and the sequential CPU model run one loop.
 * Returns the slot index, or -1 when the probe sequence covered the whole
 * table (the host doubles it and reruns). *claimed = this call filled it. */
template <typename Load, typename Cas, typename TupleOf>
COPR_GK_HD inline int64_t gk_probe(const GkTuple &t, int k, uint64_t row,
                                   uint32_t mask, Load load, Cas cas,
                                   TupleOf tuple_of, bool *claimed) {
  const uint64_t h = gk_tuple_hash(t, k);
  const uint32_t fp = gk_hash_fp(h);
  const uint64_t mine = gk_slot_pack(fp, row);
  uint32_t slot = gk_hash_slot(h, mask);
  *claimed = false;
  for (uint64_t probe = 0; probe <= (uint64_t)mask; probe++) {
    uint64_t w = load(slot);
    if (w == 0) {
      w = cas(slot, mine);
      if (w == 0) {
        *claimed = true;
        return (int64_t)slot;
      }
    }
    if (gk_slot_fp(w) == fp) {
      const uint64_t rep = gk_slot_row(w);
      if (rep == row) return (int64_t)slot;
      GkTuple o = tuple_of(rep);
      if (gk_tuple_eq(t, o, k)) return (int64_t)slot;
    }
    slot = (slot + 1) & mask;
  }
  return -1;
}

/* one key of a multi-key group-by request, and where stage 1 reads it */
struct GroupKey {
  int64_t col_id;
  int32_t uns;            /* column UNSIGNED flag (output datum form) */
  int32_t missing_null;   /* absent cell: NULL, else missing_val */
  int32_t col_off;        /* scan-column offset (host bookkeeping) */
  int32_t pad_;
  int64_t missing_val;
};

}  // namespace copr

#endif
