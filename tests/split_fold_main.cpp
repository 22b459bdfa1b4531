/* Stand-alone check of split_fc_fold and split_row_in
 * (tikv_amd/csrc/plane_fold.h) against the 32-bit narrow test,
 * and of that against the 64-bit reference (plane_fc_fold plus k_plane_fc's
 * row expression) and a direct signed / unsigned comparison. Built and run by
 * tests/test_split_fold_cpu.py with the host compiler and
 * -fsanitize=address,undefined. Exit 0 = every case agrees. */
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../tikv_amd/csrc/plane_fold.h"

using namespace copr;

static bool direct(int cmp, bool uns, int64_t v, int64_t c) {
  int r;
  if (uns) r = (uint64_t)v < (uint64_t)c ? -1 : (uint64_t)v > (uint64_t)c;
  else r = v < c ? -1 : v > c;
  switch (cmp) {
    case CMP_LT: return r < 0;
    case CMP_LE: return r <= 0;
    case CMP_GT: return r > 0;
    case CMP_GE: return r >= 0;
    case CMP_EQ: return r == 0;
    default:     return r != 0;
  }
}

static unsigned long long bad = 0;

static void fail(const char *what, int64_t base, uint64_t nmax, int uns,
                 int cmp, int cnull, int64_t c, uint64_t n) {
  if (bad++ < 20)
    fprintf(stderr, "%s: base %lld nmax %llu uns %d cmp %d null %d c %lld "
            "n %llu\n", what, (long long)base, (unsigned long long)nmax, uns,
            cmp, cnull, (long long)c, (unsigned long long)n);
}

/* n +- 2, inside [0, nmax] */
static void around(std::vector<uint64_t> *ns, uint64_t n, uint64_t nmax) {
  for (int d = -2; d <= 2; d++) {
    const int64_t x = (int64_t)n + d;
    if (x >= 0 && (uint64_t)x <= nmax) ns->push_back((uint64_t)x);
  }
}

int main() {
  const int64_t I_MIN = INT64_MIN, I_MAX = INT64_MAX;
  const int64_t bases[] = {I_MIN, -3, 0, I_MAX - 0xFFFFFFFFll};
  const uint64_t nmaxes[] = {0x10000, 0x1FFFF, 0x30000, 0xFFFFFFFFull};
  const uint32_t lows[] = {0x0000, 0x0001, 0x0002, 0xFFFD, 0xFFFE, 0xFFFF};
  unsigned long long checked = 0, declined = 0, folds = 0;
  unsigned long long empty_sure = 0, full_sure = 0;
  for (int64_t base : bases)
    for (uint64_t nmax : nmaxes) {
      if (nmax > (uint64_t)I_MAX - (uint64_t)base) continue;  /* no such plane */
      const int64_t top = (int64_t)((uint64_t)base + nmax);
      /* constants: base + t for t with every interesting low half in the
         bottom, second, middle, last-but-one and top bucket, so that after
         the comparer's +-1 the folded a and b take the low halves 0x0000,
         0x0001, 0xFFFE and 0xFFFF; EQ and NE give equal high halves; the
         extremes and the values beside the plane give empty and full
         intersections */
      std::vector<int64_t> consts = {I_MIN, I_MIN + 1, -1, 0, 1, I_MAX - 1,
                                     I_MAX};
      if (base > I_MIN) consts.push_back(base - 1);
      if (top < I_MAX) consts.push_back(top + 1);
      const uint64_t hmax = nmax >> 16;
      const uint64_t hs[] = {0, 1, hmax / 2, hmax - 1, hmax};
      for (uint64_t hh : hs)
        for (uint32_t low : lows) {
          const uint64_t t = (hh << 16) | low;
          if (t <= nmax) consts.push_back((int64_t)((uint64_t)base + t));
        }
      for (int uns = 0; uns < 2; uns++)
        for (int cmp = CMP_LT; cmp <= CMP_NE; cmp++)
          for (int cnull = 0; cnull < 2; cnull++)
            for (int64_t c : consts) {
              PlaneFcArgs fa;
              plane_fc_fold(cmp, c, uns != 0, cnull != 0, true, 0, &fa);
              NarrowFcArgs nf;
              if (!narrow_fc_fold(fa, base, nmax, uns != 0, &nf)) {
                if (!(uns && (base < 0) != (top < 0)))
                  fail("declined", base, nmax, uns, cmp, cnull, c, 0);
                declined++;
                continue;
              }
              if ((uint64_t)nf.lo + nf.span > 0xFFFFFFFFull)
                fail("wraps", base, nmax, uns, cmp, cnull, c, 0);
              SplitFcArgs sf, sa;
              split_fc_fold(nf, false, &sf);
              split_fc_fold(nf, true, &sa);      /* COPR_SPLIT_ALL_LO */
              folds++;
              const uint32_t a = nf.lo, b = nf.lo + nf.span;
              if (sf.sure_lo > 0xFFFFu) empty_sure++;
              if (sf.sure_lo == 0 && sf.sure_span == 0xFFFFu) full_sure++;
              /* "never" and "always" must not need a low half anywhere */
              if (nf.lo == 0 && nf.span == 0xFFFFFFFFu &&
                  !(sf.sure_lo == 0 && sf.sure_span == 0xFFFFu))
                fail("full range not sure", base, nmax, uns, cmp, cnull, c, 0);
              /* stored values: +-2 around a and b, around every multiple of
                 65536 adjacent to them, 0 and nmax */
              std::vector<uint64_t> ns = {0, nmax};
              for (uint64_t e : {(uint64_t)a, (uint64_t)b}) {
                around(&ns, e, nmax);
                const uint64_t m = e & ~0xFFFFull;
                around(&ns, m, nmax);
                around(&ns, m + 0x10000, nmax);
                if (m >= 0x10000) around(&ns, m - 0x10000, nmax);
              }
              std::sort(ns.begin(), ns.end());
              ns.erase(std::unique(ns.begin(), ns.end()), ns.end());
              for (uint64_t n : ns) {
                const int64_t v = (int64_t)((uint64_t)base + n);
                const unsigned long long key = (unsigned long long)v ^ fa.bias;
                const bool ref = ((key - fa.lo) <= fa.span) != (fa.invert != 0);
                const bool dir = cnull ? false : direct(cmp, uns != 0, v, c);
                const uint32_t n32 = (uint32_t)n;
                const bool full = (uint32_t)(n32 - nf.lo) <= nf.span;
                const bool nar = full != (nf.invert != 0);
                const uint32_t h = n32 >> 16, l = n32 & 0xFFFFu;
                const bool spl = split_row_in(h, l, sf) != (sf.invert != 0);
                const bool all = split_row_in(h, l, sa) != (sa.invert != 0);
                checked++;
                if (spl != nar || all != nar || nar != ref || ref != dir)
                  fail("row", base, nmax, uns, cmp, cnull, c, n);
                /* interval property, for this h and both ends of its bucket */
                if (split_sure(h, sf) && !split_maybe(h, sf))
                  fail("sure outside maybe", base, nmax, uns, cmp, cnull, c, n);
                for (uint32_t ll : {0u, l, 0xFFFFu}) {
                  const bool f = split_full_in(h, ll, sf);
                  if (split_sure(h, sf) && !f)
                    fail("sure row fails", base, nmax, uns, cmp, cnull, c, n);
                  if (!split_maybe(h, sf) && f)
                    fail("row outside maybe passes", base, nmax, uns, cmp,
                         cnull, c, n);
                }
                /* the switch: every row open, none sure */
                if (!split_maybe(h, sa) || split_sure(h, sa))
                  fail("all_lo", base, nmax, uns, cmp, cnull, c, n);
              }
            }
    }
  /* the two fixed encodings over every h: an empty sure interval holds no
     h <= 0xFFFF, and the all_lo fold leaves every h open */
  {
    NarrowFcArgs nf = {0x12345, 0x10, 0};      /* a and b inside one bucket */
    SplitFcArgs sf, sa;
    split_fc_fold(nf, false, &sf);
    split_fc_fold(nf, true, &sa);
    for (uint32_t h = 0; h <= 0xFFFFu; h++) {
      if (split_sure(h, sf) || split_sure(h, sa) || !split_maybe(h, sa) ||
          split_maybe(h, sf) != (h == 1))
        bad++;
    }
  }
  if (!empty_sure || !full_sure) {
    fprintf(stderr, "cases missing: %llu empty, %llu full sure intervals\n",
            empty_sure, full_sure);
    bad++;
  }
  printf("split fold: %llu folds, %llu row checks, %llu declined folds, "
         "%llu mismatches\n", folds, checked, declined, bad);
  return bad ? 1 : 0;
}
