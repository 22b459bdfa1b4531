/* Stand-alone check of the packed interval count (tikv_amd/csrc/plane_fold.h
 * fold_packed_out and the packed fields split_fc_fold fills)
 * against split_maybe and split_sure, the per-row tests it stands in for.
 * Built and run by tests/test_packed_fold_cpu.py with the host compiler and
 * -fsanitize=address,undefined. Exit 0 = every case agrees. */
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../tikv_amd/csrc/plane_fold.h"

using namespace copr;

static unsigned long long bad = 0, checked = 0, folds = 0;
static unsigned long long n_empty = 0, n_open = 0;

static void fail(const char *what, const NarrowFcArgs &nf, int all_lo,
                 uint32_t h0, uint32_t h1) {
  if (bad++ < 20)
    fprintf(stderr, "%s: lo %#x span %#x invert %u all_lo %d halves %#x %#x\n",
            what, nf.lo, nf.span, nf.invert, all_lo, h0, h1);
}

/* the rows the kernel's fast path counts outside the sure interval */
static uint32_t out_sure_of(uint32_t w, const SplitFcArgs &sf) {
  return sf.sure_empty ? 2u
                       : fold_packed_out(w, sf.sure_lo_pk, sf.sure_span_pk);
}

static void add_half(std::vector<uint32_t> *hs, int64_t h) {
  for (int d = -1; d <= 1; d++)
    if (h + d >= 0 && h + d <= 0xFFFF) hs->push_back((uint32_t)(h + d));
}

static void check_fold(const NarrowFcArgs &nf, int all_lo) {
  SplitFcArgs sf;
  split_fc_fold(nf, all_lo != 0, &sf);
  folds++;
  const bool empty32 = sf.sure_lo == 0x10000u && sf.sure_span == 0;
  if ((sf.sure_empty != 0) != empty32) fail("sure_empty", nf, all_lo, 0, 0);
  if (sf.sure_empty > 1) fail("sure_empty not 0/1", nf, all_lo, 0, 0);
  if (empty32) n_empty++;
  if (sf.maybe_lo > 0xFFFFu || sf.maybe_lo + sf.maybe_span > 0xFFFFu ||
      sf.maybe_lo_pk != sf.maybe_lo * 0x10001u ||
      sf.maybe_span_pk != sf.maybe_span * 0x10001u)
    fail("maybe packing", nf, all_lo, 0, 0);
  if (!empty32 &&
      (sf.sure_lo + sf.sure_span > 0xFFFFu ||
       sf.sure_lo_pk != sf.sure_lo * 0x10001u ||
       sf.sure_span_pk != sf.sure_span * 0x10001u))
    fail("sure packing", nf, all_lo, 0, 0);
  /* halves: both ends of both intervals +-1, 0 and 0xFFFF */
  std::vector<uint32_t> hs = {0, 0xFFFFu};
  add_half(&hs, sf.maybe_lo);
  add_half(&hs, (int64_t)sf.maybe_lo + sf.maybe_span);
  if (!empty32) {
    add_half(&hs, sf.sure_lo);
    add_half(&hs, (int64_t)sf.sure_lo + sf.sure_span);
  }
  std::sort(hs.begin(), hs.end());
  hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
  for (uint32_t h0 : hs)
    for (uint32_t h1 : hs) {
      const uint32_t w = h0 | (h1 << 16);
      const uint32_t om = fold_packed_out(w, sf.maybe_lo_pk, sf.maybe_span_pk);
      const uint32_t os = out_sure_of(w, sf);
      const uint32_t ref_m = (split_maybe(h0, sf) ? 0u : 1u) +
                             (split_maybe(h1, sf) ? 0u : 1u);
      const uint32_t ref_s = (split_sure(h0, sf) ? 0u : 1u) +
                             (split_sure(h1, sf) ? 0u : 1u);
      checked++;
      if (om != ref_m) fail("out_maybe", nf, all_lo, h0, h1);
      if (os != ref_s) fail("out_sure", nf, all_lo, h0, h1);
      const bool open = (split_maybe(h0, sf) && !split_sure(h0, sf)) ||
                        (split_maybe(h1, sf) && !split_sure(h1, sf));
      if (open) n_open++;
      if ((os != om) != open) fail("open-lane rule", nf, all_lo, h0, h1);
    }
}

int main() {
  std::vector<uint32_t> ends = {0u, 1u, 0xFFFFu, 0x10000u, 0x10001u,
                                0x7FFF0000u, 0xFFFEFFFFu, 0xFFFF0000u,
                                0xFFFFFFFFu};
  uint64_t s = 0x9E3779B97F4A7C15ull;             /* seeded: xorshift64* */
  for (int i = 0; i < 40; i++) {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    uint32_t x = (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    /* a third of them a few buckets wide, so that random pairs also give
       intervals inside one bucket and next to a bucket's end */
    if (i % 3 == 0) x &= 0x3FFFFu;
    ends.push_back(x);
  }
  for (uint32_t a : ends)
    for (uint32_t b : ends) {
      if (a > b) continue;
      for (uint32_t inv = 0; inv < 2; inv++)
        for (int all_lo = 0; all_lo < 2; all_lo++) {
          const NarrowFcArgs nf = {a, b - a, inv};
          check_fold(nf, all_lo);
        }
    }
  /* narrow_fc_fold's "never": the whole range, inverted */
  for (int all_lo = 0; all_lo < 2; all_lo++) {
    const NarrowFcArgs never = {0, 0xFFFFFFFFu, 1};
    check_fold(never, all_lo);
  }
  /* the packed steps themselves on the extremes of a half */
  if (fold_pk_sub_u16(0x00000000u, 0x00010001u) != 0xFFFFFFFFu ||
      fold_pk_sub_u16(0x00010000u, 0x00000001u) != 0x0001FFFFu ||
      fold_pk_sub_sat_u16(0x0000FFFFu, 0x0001FFFEu) != 0x00000001u ||
      fold_pk_min_u16(0xFFFF0000u, 0x00010001u) != 0x00010000u ||
      fold_pack16(0x1FFFFu) != 0xFFFFFFFFu || fold_pack16(0x12u) != 0x00120012u)
    bad++;
  if (!n_empty || !n_open) {
    fprintf(stderr, "cases missing: %llu empty sure, %llu open pairs\n",
            n_empty, n_open);
    bad++;
  }
  printf("packed fold: %llu folds, %llu pair checks, %llu mismatches\n", folds,
         checked, bad);
  return bad ? 1 : 0;
}
