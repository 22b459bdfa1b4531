/* Stand-alone check of plane_fc_and (tikv_amd/csrc/plane_fold.h).
 * Part one: every pair of the six comparers, both signednesses, NULL and
 * non-NULL constants, constants and values around 0, the sign boundary and
 * both 64-bit ends. A fold that succeeds keeps exactly the values (and the
 * ABSENT fill) both conditions keep by direct comparison; it is refused only
 * for an NE point strictly inside the other side's interval or two different
 * NE points, neither side empty. Part two: the folded test through
 * narrow_fc_fold, split_fc_fold and bucket_fc_fold over a small plane against
 * the per-row AND. Built with -fsanitize=address,undefined and run by
 * tests/test_pair_fold_cpu.py. Exit 0 = every case agrees. */
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../tikv_amd/csrc/plane_fold.h"

using namespace copr;
typedef __int128 i128;

struct Cond { int cmp; bool cnull; int64_t c; };

static i128 ord(bool uns, int64_t v) { return uns ? (i128)(uint64_t)v : (i128)v; }

static bool direct(const Cond &k, bool uns, int64_t v) {
  const i128 a = ord(uns, v), b = ord(uns, k.c);
  if (k.cnull) return false;
  switch (k.cmp) {
    case CMP_LT: return a < b;
    case CMP_LE: return a <= b;
    case CMP_GT: return a > b;
    case CMP_GE: return a >= b;
    case CMP_EQ: return a == b;
    default:     return a != b;
  }
}

/* is p strictly inside the non-empty interval a non-NE condition keeps? */
static bool strictly_inside(const Cond &k, bool uns, i128 p) {
  i128 lo = uns ? (i128)0 : (i128)INT64_MIN;
  i128 hi = uns ? (i128)UINT64_MAX : (i128)INT64_MAX;
  const i128 c = ord(uns, k.c);
  switch (k.cmp) {
    case CMP_LT: hi = c - 1; break;
    case CMP_LE: hi = c; break;
    case CMP_GT: lo = c + 1; break;
    case CMP_GE: lo = c; break;
    default:     lo = hi = c; break;
  }
  return !k.cnull && lo < p && p < hi;
}

static unsigned long long bad = 0;
static void fail(const char *what, int uns, const Cond &a, const Cond &b) {
  if (bad++ < 20)
    fprintf(stderr, "%s: uns %d, cmp %d null %d c %lld AND cmp %d null %d c %lld\n",
            what, uns, a.cmp, (int)a.cnull, (long long)a.c, b.cmp,
            (int)b.cnull, (long long)b.c);
}

int main() {
  const int64_t I_MIN = INT64_MIN, I_MAX = INT64_MAX;
  const int64_t pts[] = {I_MIN, I_MIN + 1, I_MIN + 2, -2, -1, 0, 1, 2,
                         I_MAX - 2, I_MAX - 1, I_MAX};
  unsigned long long folded = 0, refused = 0;
  std::vector<Cond> conds;
  for (int cmp = CMP_LT; cmp <= CMP_NE; cmp++) {
    for (int64_t c : pts) conds.push_back({cmp, false, c});
    conds.push_back({cmp, true, 0});
  }
  for (int u = 0; u < 2; u++)
    for (const Cond &a : conds)
      for (const Cond &b : conds)
        for (int64_t miss : {(int64_t)0, I_MIN, I_MAX}) {
          const bool uns = u != 0;
          PlaneFcArgs fa, fb, out;
          plane_fc_fold(a.cmp, a.c, uns, a.cnull, false, miss, &fa);
          plane_fc_fold(b.cmp, b.c, uns, b.cnull, false, miss, &fb);
          auto both = [&](int64_t v) { return direct(a, uns, v) && direct(b, uns, v); };
          if (plane_fc_and(fa, fb, &out)) {
            folded++;
            for (int64_t v : pts) {
              const unsigned long long key = (unsigned long long)v ^ out.bias;
              if ((((key - out.lo) <= out.span) != (out.invert != 0)) != both(v))
                fail("value", u, a, b);
            }
            if ((out.keep_absent != 0) != both(miss)) fail("absent", u, a, b);
            if (out.bias != fa.bias || out.lo + out.span < out.lo)
              fail("form", u, a, b);
            continue;
          }
          refused++;
          const bool a_ne = a.cmp == CMP_NE, b_ne = b.cmp == CMP_NE;
          bool named = false;
          if (a_ne && b_ne)
            named = !a.cnull && !b.cnull && a.c != b.c;
          else if (a_ne != b_ne)
            named = !(a_ne ? a : b).cnull &&
                    strictly_inside(a_ne ? b : a, uns, ord(uns, (a_ne ? a : b).c));
          if (!named) fail("refused", u, a, b);
        }
  /* part two: 600 rows over buckets 0 .. 2; cuts in one bucket, in adjacent
     buckets, far apart, on stored values and on the plane's ends */
  for (int64_t base : {I_MIN, (int64_t)-70000, (int64_t)0, I_MAX - 0x2FFFF}) {
    const uint64_t nmax = 0x2FFFF, n_rows = 600;
    const bool uns = base >= 0;
    std::vector<uint32_t> ns(n_rows);
    for (uint64_t i = 0; i < n_rows; i++)
      ns[i] = (uint32_t)((i * 7919u * 31u) % (nmax + 1));
    ns[0] = 0;
    ns[n_rows - 1] = (uint32_t)nmax;
    std::vector<uint64_t> off(COPR_N_BUCKETS + 1, 0);
    for (uint32_t n : ns) off[(n >> 16) + 1]++;
    for (uint32_t h = 0; h < COPR_N_BUCKETS; h++) off[h + 1] += off[h];
    std::vector<uint16_t> bkt(n_rows);
    std::vector<uint64_t> fill(off.begin(), off.end() - 1);
    for (uint32_t n : ns) bkt[fill[n >> 16]++] = (uint16_t)n;
    const uint64_t cuts[] = {0, 1, ns[7], 0x8000, 0xFFFF, 0x10000, 0x10001,
                             ns[11], 0x1FFFF, 0x20000, 0x28000, nmax - 1, nmax};
    for (int ca = CMP_LT; ca <= CMP_NE; ca++)
      for (int cb = CMP_LT; cb <= CMP_NE; cb++)
        for (uint64_t ta : cuts)
          for (uint64_t tb : cuts) {
            const Cond a = {ca, false, (int64_t)((uint64_t)base + ta)};
            const Cond b = {cb, false, (int64_t)((uint64_t)base + tb)};
            PlaneFcArgs fa, fb, out;
            NarrowFcArgs nf;
            SplitFcArgs sf;
            BucketFcArgs ba;
            plane_fc_fold(a.cmp, a.c, uns, false, true, 0, &fa);
            plane_fc_fold(b.cmp, b.c, uns, false, true, 0, &fb);
            if (!plane_fc_and(fa, fb, &out)) continue;
            if (!narrow_fc_fold(out, base, nmax, uns, &nf)) {
              fail("narrow refused", uns, a, b);
              continue;
            }
            split_fc_fold(nf, false, &sf);
            if (!bucket_fc_fold(sf, off.data(), n_rows, &ba)) {
              fail("bucket refused", uns, a, b);
              continue;
            }
            uint64_t in = ba.sure, c_nar = 0, c_split = 0, c_dir = 0;
            for (uint32_t s = 0; s < ba.n_slices; s++)
              for (uint64_t i = ba.beg[s]; i < ba.end[s]; i++)
                in += split_full_in(ba.h[s], bkt[i], sf) ? 1u : 0u;
            for (uint32_t n : ns) {
              const int64_t v = (int64_t)((uint64_t)base + n);
              c_nar += (((n - nf.lo) <= nf.span) != (nf.invert != 0)) ? 1u : 0u;
              c_split += (split_row_in(n >> 16, n & 0xFFFFu, sf) !=
                          (sf.invert != 0)) ? 1u : 0u;
              c_dir += (direct(a, uns, v) && direct(b, uns, v)) ? 1u : 0u;
            }
            if (c_nar != c_dir || c_split != c_dir ||
                (ba.invert ? n_rows - in : in) != c_dir)
              fail("count", uns, a, b);
          }
  }
  if (!folded || !refused) bad++;
  printf("pair fold: %llu folded, %llu refused, %llu mismatches\n", folded,
         refused, bad);
  return bad ? 1 : 0;
}
