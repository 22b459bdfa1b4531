/* Stand-alone check of narrow_fc_fold (tikv_amd/csrc/plane_fold.h) against
 * the 64-bit reference: plane_fc_fold plus k_plane_fc's row expression, and
 * against a direct signed / unsigned comparison. Built and run by
 * tests/test_narrow_fold_cpu.py with the host compiler and
 * -fsanitize=address,undefined. Exit 0 = every case agrees. */
#include <stdint.h>
#include <stdio.h>
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

int main() {
  const int64_t I_MIN = INT64_MIN, I_MAX = INT64_MAX;
  const int64_t bases[] = {I_MIN, -3, 0, I_MAX - 300};
  const uint64_t nmaxes[] = {0, 1, 255, 256, 65535};
  unsigned long long checked = 0, declined = 0, bad = 0;
  for (int64_t base : bases)
    for (uint64_t nmax : nmaxes) {
      if (nmax > (uint64_t)I_MAX - (uint64_t)base) continue;  /* no such plane */
      const int64_t top = (int64_t)((uint64_t)base + nmax);
      /* constants: a grid around both edges, plus the extremes */
      std::vector<int64_t> consts = {I_MIN, I_MIN + 1, -1, 0, 1, I_MAX - 1, I_MAX};
      for (int d = -3; d <= 3; d++) {
        consts.push_back((int64_t)((uint64_t)base + (uint64_t)(int64_t)d));
        consts.push_back((int64_t)((uint64_t)top + (uint64_t)(int64_t)d));
        consts.push_back((int64_t)((uint64_t)base + nmax / 2 + (uint64_t)(int64_t)d));
      }
      /* stored values: all of them up to a few hundred, else both ends and
         the middle */
      std::vector<uint64_t> ns;
      if (nmax <= 600) {
        for (uint64_t n = 0; n <= nmax; n++) ns.push_back(n);
      } else {
        for (uint64_t n = 0; n < 200; n++) {
          ns.push_back(n);
          ns.push_back(nmax - n);
          ns.push_back(nmax / 2 - 100 + n);
        }
      }
      for (int uns = 0; uns < 2; uns++)
        for (int cmp = CMP_LT; cmp <= CMP_NE; cmp++)
          for (int cnull = 0; cnull < 2; cnull++)
            for (int64_t c : consts) {
              PlaneFcArgs fa;
              plane_fc_fold(cmp, c, uns != 0, cnull != 0, true, 0, &fa);
              NarrowFcArgs nf;
              const bool ok = narrow_fc_fold(fa, base, nmax, uns != 0, &nf);
              const bool want_ok = !(uns && (base < 0) != (top < 0));
              if (ok != want_ok) {
                bad++;
                fprintf(stderr, "usable=%d want %d: base %lld nmax %llu uns %d\n",
                        ok, want_ok, (long long)base, (unsigned long long)nmax, uns);
                continue;
              }
              if (!ok) { declined++; continue; }
              for (uint64_t n : ns) {
                const int64_t v = (int64_t)((uint64_t)base + n);
                const unsigned long long key = (unsigned long long)v ^ fa.bias;
                const bool ref = ((key - fa.lo) <= fa.span) != (fa.invert != 0);
                const bool dir = cnull ? false : direct(cmp, uns != 0, v, c);
                const uint32_t n32 = (uint32_t)n;
                const bool got =
                    ((uint32_t)(n32 - nf.lo) <= nf.span) != (nf.invert != 0);
                checked++;
                if (got != ref || ref != dir) {
                  if (bad++ < 20)
                    fprintf(stderr,
                            "base %lld nmax %llu uns %d cmp %d null %d c %lld "
                            "n %llu: narrow %d wide %d direct %d\n",
                            (long long)base, (unsigned long long)nmax, uns, cmp,
                            cnull, (long long)c, (unsigned long long)n, got, ref,
                            dir);
                }
              }
            }
    }
  /* a range of 2^32 or more is never usable */
  {
    PlaneFcArgs fa;
    NarrowFcArgs nf;
    plane_fc_fold(CMP_LT, 0, false, false, true, 0, &fa);
    if (narrow_fc_fold(fa, 0, 0x100000000ull, false, &nf)) bad++;
    if (!narrow_fc_fold(fa, -5, 0xFFFFFFFFull, false, &nf)) bad++;
  }
  printf("narrow fold: %llu row checks, %llu declined folds, %llu mismatches\n",
         checked, declined, bad);
  return bad ? 1 : 0;
}
