/* Stand-alone check of bucket_fc_fold (tikv_amd/csrc/plane_fold.h, DESIGN
 * §9q) and the slice rule of k_plane_fcb,
 *   in = sure + #{l in slice : split_full_in(h, l)},
 *   count = invert ? n_rows - in : in,
 * against split_row_in row by row, and of that against the 64-bit reference
 * (plane_fc_fold plus k_plane_fc's row expression) and a direct signed /
 * unsigned comparison. Columns of 1 to 300 random values spread over one
 * bucket, two adjacent buckets and wide ranges; the offsets and the grouped
 * low halves are built here on the host. Built and run by
 * tests/test_bucket_fold_cpu.py with the host compiler and
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {              /* xorshift64* */
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static unsigned long long bad = 0;

static void fail(const char *what, int64_t base, uint64_t nmax, int uns,
                 int cmp, int cnull, int64_t c) {
  if (bad++ < 20)
    fprintf(stderr, "%s: base %lld nmax %llu uns %d cmp %d null %d c %lld\n",
            what, (long long)base, (unsigned long long)nmax, uns, cmp, cnull,
            (long long)c);
}

int main() {
  const int64_t I_MIN = INT64_MIN, I_MAX = INT64_MAX;
  const int64_t bases[] = {I_MIN, -70000, 0, I_MAX - 0xFFFFFFFFll};
  /* the spread of the stored n: inside one bucket, over two adjacent
     buckets, a few buckets, the whole 32-bit domain. A one-sided comparer
     folds to [0, x] or [x, nmax], so two slices need an nmax whose low half
     is not 0xFFFF */
  const uint64_t spreads[] = {0x0FFF, 0xFFFF, 0x1F000, 0x1FFFF, 0x5F123,
                              0xFFFFFFFFull};
  unsigned long long folds = 0, rows = 0, declined = 0;
  unsigned long long never_forms = 0, one_slice = 0, two_slices = 0,
                     no_slice = 0, empty_slices = 0;
  for (int64_t base : bases)
    for (uint64_t spread : spreads)
      for (int rep = 0; rep < 6; rep++) {
        /* a column of n_rows values n in [0, spread], min and max
           present so that the plane's base and nmax are known */
        const uint64_t n_rows = 1 + rnd() % 300;
        std::vector<uint32_t> ns(n_rows);
        for (uint64_t i = 0; i < n_rows; i++)
          ns[i] = (uint32_t)(rnd() % (spread + 1));
        ns[0] = 0;
        if (n_rows > 1) ns[n_rows - 1] = (uint32_t)spread;
        const uint64_t nmax = n_rows > 1 ? spread : 0;
        if (nmax > (uint64_t)I_MAX - (uint64_t)base) continue;
        const int64_t top = (int64_t)((uint64_t)base + nmax);
        /* the index: offsets by counting, low halves grouped by h; inside a
           bucket in reverse row order, since the order must not matter */
        std::vector<uint64_t> off(COPR_N_BUCKETS + 1, 0);
        for (uint32_t n : ns) off[(n >> 16) + 1]++;
        for (uint32_t h = 0; h < COPR_N_BUCKETS; h++) off[h + 1] += off[h];
        std::vector<uint16_t> bkt(n_rows);
        {
          std::vector<uint64_t> fill(off.begin(), off.end() - 1);
          for (uint64_t i = n_rows; i-- > 0;)
            bkt[fill[ns[i] >> 16]++] = (uint16_t)ns[i];
        }
        /* constants: c - 1, c, c + 1 around every bucket bound that holds or
           neighbours a row, around min and max, and the extremes */
        std::vector<int64_t> consts = {I_MIN, I_MIN + 1, -1, 0, 1, I_MAX - 1,
                                       I_MAX};
        auto add3 = [&](uint64_t t) {
          for (int d = -1; d <= 1; d++) {
            const __int128 v = (__int128)base + (__int128)t + d;
            if (v >= I_MIN && v <= I_MAX) consts.push_back((int64_t)v);
          }
        };
        add3(0);
        add3(nmax);
        const uint64_t hmax = nmax >> 16;
        const uint64_t hs[] = {0, 1, 2, hmax / 2, hmax > 0 ? hmax - 1 : 0,
                               hmax, hmax + 1};
        for (uint64_t hh : hs) {
          add3(hh << 16);                 /* low half 0x0000 */
          add3((hh << 16) | 0xFFFF);      /* low half 0xFFFF */
        }
        for (int k = 0; k < 4; k++) add3(ns[rnd() % n_rows]);
        for (int uns = 0; uns < 2; uns++)
          for (int cmp = CMP_LT; cmp <= CMP_NE; cmp++)
            for (int cnull = 0; cnull < 2; cnull++)
              for (int64_t c : consts) {
                PlaneFcArgs fa;
                plane_fc_fold(cmp, c, uns != 0, cnull != 0, true, 0, &fa);
                NarrowFcArgs nf;
                if (!narrow_fc_fold(fa, base, nmax, uns != 0, &nf)) {
                  if (!(uns && (base < 0) != (top < 0)))
                    fail("declined", base, nmax, uns, cmp, cnull, c);
                  declined++;
                  continue;
                }
                SplitFcArgs sf;
                split_fc_fold(nf, false, &sf);
                BucketFcArgs ba;
                if (!bucket_fc_fold(sf, off.data(), n_rows, &ba)) {
                  fail("fold refused", base, nmax, uns, cmp, cnull, c);
                  continue;
                }
                folds++;
                if (ba.invert != sf.invert || ba.n_slices > 2)
                  fail("shape", base, nmax, uns, cmp, cnull, c);
                const bool same_h = (nf.lo >> 16) == ((nf.lo + nf.span) >> 16);
                if (same_h && ba.n_slices > 1)
                  fail("two slices for one bucket", base, nmax, uns, cmp,
                       cnull, c);
                if (nf.lo == 0 && nf.span == 0xFFFFFFFFu) {
                  /* "never" and "always": every row sure, no slice */
                  never_forms += nf.invert ? 1 : 0;
                  if (ba.sure != n_rows || ba.n_slices != 0)
                    fail("full range", base, nmax, uns, cmp, cnull, c);
                }
                (ba.n_slices == 0 ? no_slice
                 : ba.n_slices == 1 ? one_slice : two_slices)++;
                /* the slice rule */
                uint64_t in = ba.sure, slice_rows = 0;
                for (uint32_t s = 0; s < ba.n_slices; s++) {
                  if (ba.beg[s] > ba.end[s] || ba.end[s] > n_rows ||
                      ba.beg[s] != off[ba.h[s]] ||
                      ba.end[s] != off[ba.h[s] + 1] ||
                      !split_maybe(ba.h[s], sf) || split_sure(ba.h[s], sf)) {
                    fail("slice", base, nmax, uns, cmp, cnull, c);
                    continue;
                  }
                  if (ba.beg[s] == ba.end[s]) empty_slices++;
                  if (s == 1 && ba.h[1] == ba.h[0])
                    fail("slice twice", base, nmax, uns, cmp, cnull, c);
                  slice_rows += ba.end[s] - ba.beg[s];
                  for (uint64_t i = ba.beg[s]; i < ba.end[s]; i++)
                    in += split_full_in(ba.h[s], bkt[i], sf) ? 1u : 0u;
                }
                if (ba.sure + slice_rows > n_rows)
                  fail("more rows than the plane", base, nmax, uns, cmp,
                       cnull, c);
                const uint64_t count = ba.invert ? n_rows - in : in;
                /* row by row: split_row_in, the 64-bit reference, direct */
                uint64_t c_split = 0, c_ref = 0, c_dir = 0;
                for (uint32_t n : ns) {
                  const int64_t v = (int64_t)((uint64_t)base + n);
                  const unsigned long long key =
                      (unsigned long long)v ^ fa.bias;
                  c_split += (split_row_in(n >> 16, n & 0xFFFFu, sf) !=
                              (sf.invert != 0)) ? 1u : 0u;
                  c_ref += (((key - fa.lo) <= fa.span) != (fa.invert != 0))
                               ? 1u : 0u;
                  c_dir += (!cnull && direct(cmp, uns != 0, v, c)) ? 1u : 0u;
                  rows++;
                }
                if (count != c_split || c_split != c_ref || c_ref != c_dir)
                  fail("count", base, nmax, uns, cmp, cnull, c);
              }
      }
  /* offsets that are no offsets are refused, never followed */
  {
    NarrowFcArgs nf = {0x12345, 0x30000, 0};
    SplitFcArgs sf;
    split_fc_fold(nf, false, &sf);
    std::vector<uint64_t> off(COPR_N_BUCKETS + 1, 10);
    off[0] = 0;
    BucketFcArgs ba;
    if (!bucket_fc_fold(sf, off.data(), 10, &ba)) bad++;   /* all in h = 0 */
    off[2] = 11;                                           /* beyond n_rows */
    if (bucket_fc_fold(sf, off.data(), 10, &ba)) bad++;
    off[2] = 3;                                            /* decreasing */
    if (bucket_fc_fold(sf, off.data(), 10, &ba)) bad++;
  }
  if (!never_forms || !one_slice || !two_slices || !no_slice ||
      !empty_slices) {
    fprintf(stderr, "cases missing: never %llu, slices 0/1/2 %llu/%llu/%llu, "
            "empty %llu\n", never_forms, no_slice, one_slice, two_slices,
            empty_slices);
    bad++;
  }
  printf("bucket fold: %llu folds, %llu row checks, %llu declined folds, "
         "%llu mismatches\n", folds, rows, declined, bad);
  return bad ? 1 : 0;
}
