/* in_split_fold / in_split_row (tikv_amd/csrc/in_set.h) against
 * std::set of exact integers; stand-alone, built and run by
 * test_in_split_cpu.py */
#include <cstdio>
#include <set>
#include <vector>

#include "../tikv_amd/csrc/in_set.h"
#include "../tikv_amd/csrc/plane_fold.h"

using copr::InItem;

static long long g_checks = 0, g_bad = 0;

static void bad(const char *what, long long a, long long b) {
  if (g_bad++ < 20) printf("%s: %lld %lld\n", what, a, b);
}

static __int128 exact(uint64_t bits, bool uns) {
  return uns ? (__int128)bits : (__int128)(int64_t)bits;
}

/* one plane domain [base, base + nmax] read under probe_uns, one list */
static void check(uint64_t base, uint64_t nmax, bool probe_uns,
                  const std::vector<InItem> &items, bool expect_none) {
  const copr::InSet s = copr::in_set_build(items.data(), items.size(), probe_uns);
  const __int128 xb = exact(base, probe_uns);
  std::set<__int128> ref;
  std::set<uint32_t> ref_buckets;
  for (const InItem &it : items) {
    if (it.null) continue;
    const __int128 x = exact(it.bits, it.uns != 0);
    ref.insert(x);
    if (x >= xb && x <= xb + nmax) ref_buckets.insert((uint32_t)((x - xb) >> 16));
  }
  copr::InSplitArgs sa;
  std::vector<uint32_t> bm;
  copr::in_split_fold(s, (int64_t)base, nmax, &sa, &bm);
  g_checks++;
  if (sa.flagged != ref_buckets.size() || sa.buckets != (nmax >> 16) + 1)
    bad("flagged", sa.flagged, sa.buckets);
  if ((sa.none != 0) != ref_buckets.empty() || (sa.none != 0) != expect_none)
    bad("none", sa.none, (long long)ref_buckets.size());
  /* the bitmap is the reference's buckets; the hull is their tight interval,
     and its packed constants classify every h as the scalar interval does */
  if (bm.size() != (nmax >> 21) + 1) bad("bitmap words", (long long)bm.size(), 0);
  for (uint32_t h = 0; h <= (uint32_t)(nmax >> 16); h++) {
    g_checks++;
    if ((((bm[h >> 5] >> (h & 31)) & 1) != 0) != (ref_buckets.count(h) != 0))
      bad("bucket bit", h, 0);
  }
  if (!sa.none) {
    if (sa.hull_lo != *ref_buckets.begin() ||
        sa.hull_lo + sa.hull_span != *ref_buckets.rbegin())
      bad("hull", sa.hull_lo, sa.hull_span);
    for (uint32_t h = 0; h <= 0xFFFFu; h++) {
      const uint32_t out = (h - sa.hull_lo) <= sa.hull_span ? 0u : 2u;
      g_checks++;
      if (copr::fold_packed_out(h * 0x10001u, sa.hull_lo_pk, sa.hull_span_pk) != out)
        bad("packed hull", h, out);
    }
  }
  /* probes: every key, key +- 1, key +- 65536 where a row can hold them, the
     domain's ends, and `empty` */
  std::vector<uint64_t> probes = {base, base + nmax, s.empty};
  for (const InItem &it : items)
    for (unsigned long long d : {0ull, 1ull, ~0ull, 65536ull, ~65535ull})
      probes.push_back(it.bits + d);
  const bool has_null = s.has_null;
  for (uint64_t v : probes) {
    const uint64_t n = v - base;
    if (n > nmax) continue;
    const uint32_t h = (uint32_t)(n >> 16), l = (uint32_t)(n & 0xFFFFu);
    const bool hit = ref.count(xb + n) != 0;
    for (uint32_t negate = 0; negate < 2; negate++) {
      const uint32_t never = (negate && has_null) ? 1u : 0u;
      const bool want = !never && hit != (negate != 0);
      g_checks++;
      if (copr::in_split_row(h, l, bm.data(), s.tab.data(), s.mask, s.empty,
                             base, negate, never) != want)
        bad("row", (long long)n, want);
    }
  }
}

int main() {
  const uint64_t BASES[] = {(uint64_t)-3ll, (uint64_t)-1000000000ll,
                            (uint64_t)INT64_MAX - (1ull << 31)};
  const uint64_t NMAX[] = {0x10000ull, 70000ull, 2000000000ull, 0xFFFFFFFFull};
  for (uint64_t base : BASES) {
    for (uint64_t nmax : NMAX) {
      for (int pu = 0; pu < 2; pu++) {
        /* the plane's rows are values of the column: a signed one ends by
           INT64_MAX, an unsigned one starts at 0 or above */
        if (!pu && (int64_t)(base + nmax) < (int64_t)base) continue;
        if (pu && (int64_t)base < 0) continue;
        const uint8_t k = (uint8_t)pu;          /* the probe's own kind */
        std::vector<InItem> edge, none;
        const uint64_t in_d[] = {0, 0xFFFF, 0x10000, nmax, nmax + 1, ~0ull,
                                 5, 0x10005,             /* one L, two buckets */
                                 0x10006,                /* and one H */
                                 nmax - 0x10000};
        const uint64_t out_d[] = {~0ull, ~65535ull, nmax + 1, nmax + 65536};
        for (uint64_t d : in_d)
          edge.push_back(InItem{base + d, k, 0});
        /* unmatchable under this probe, and the other kind where it matches */
        edge.push_back(InItem{(1ull << 63) + 5, (uint8_t)!pu, 0});
        if (!((base + 7) >> 63)) edge.push_back(InItem{base + 7, (uint8_t)!pu, 0});
        check(base, nmax, pu != 0, edge, false);
        edge.push_back(InItem{0, 0, 1});                       /* NULL: never */
        check(base, nmax, pu != 0, edge, false);
        /* no key in the domain: below, above, unmatchable, NULL */
        for (uint64_t d : out_d)
          none.push_back(InItem{base + d, k, 0});
        none.push_back(InItem{(1ull << 63) + 5, (uint8_t)!pu, 0});
        check(base, nmax, pu != 0, none, true);
        none.push_back(InItem{0, 0, 1});
        check(base, nmax, pu != 0, none, true);
      }
    }
  }
  printf("%lld checks, %lld mismatches\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
