/* in_set_build / in_set_probe (tikv_amd/csrc/in_set.h) against std::set of
 * exact integers; stand-alone, built and run by test_in_set_cpu.py */
#include <cstdio>
#include <set>
#include <vector>

#include "../tikv_amd/csrc/in_set.h"

using copr::InItem;

static long long g_checks = 0, g_bad = 0;

static __int128 exact(uint64_t bits, bool uns) {
  return uns ? (__int128)bits : (__int128)(int64_t)bits;
}

static void check_list(const std::vector<InItem> &items, bool probe_uns) {
  const copr::InSet s = copr::in_set_build(items.data(), items.size(), probe_uns);
  std::set<__int128> ref;
  bool has_null = false;
  for (const InItem &it : items) {
    if (it.null) has_null = true;
    else ref.insert(exact(it.bits, it.uns != 0));
  }
  /* the image's slot count */
  uint32_t want = 16;
  while (want < 2 * s.n_keys && want < 2048) want <<= 1;
  if (s.tab.size() != want || s.mask != want - 1)
    g_bad += printf("bad image: %zu slots, %u keys\n", s.tab.size(), s.n_keys) > 0;
  /* probes: every item, every item +- 1, empty, and the edges */
  std::vector<uint64_t> probes = {s.empty, 0, ~0ull, 1ull << 63, (1ull << 63) - 1};
  for (const InItem &it : items)
    for (uint64_t d : {0ull, 1ull, ~0ull}) probes.push_back(it.bits + d);
  for (uint64_t v : probes) {
    const int want_r = ref.count(exact(v, probe_uns)) ? 1 : has_null ? -1 : 0;
    g_checks++;
    if (copr::in_set_eval(s, v) != want_r && g_bad++ < 20)
      printf("mismatch: n=%zu uns=%d v=%llu want %d\n", items.size(),
             (int)probe_uns, (unsigned long long)v, want_r);
  }
}

int main() {
  /* INT64_MIN or 2^63, -1 or 2^64-1, 0, INT64_MAX: each under both kinds */
  const uint64_t EDGE[] = {1ull << 63, ~0ull, 0, (1ull << 63) - 1};
  uint64_t rng = 0x2545F4914F6CDD1Dull;
  auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  for (int pu = 0; pu < 2; pu++) {
    for (size_t n : {1, 2, 15, 16, 17, 1023, 1024}) {
      for (int shape = 0; shape < 5; shape++) {
        std::vector<InItem> items;
        uint64_t v = 0, m = 15;
        while (m + 1 < 2 * n && m < 2047) m = 2 * m + 1;
        for (size_t i = 0; i < n; i++) {
          InItem it{};
          if (shape == 0) {          /* random, NULLs and duplicates */
            it = InItem{rnd(), (uint8_t)(rnd() & 1), (uint8_t)(i % 7 == 3)};
            if (i % 5 == 4) it = items[i / 2];
          } else if (shape == 1) {   /* the edges under both kinds, then small */
            it = i < 8 ? InItem{EDGE[i % 4], (uint8_t)(i / 4), 0}
                       : InItem{i - 8, (uint8_t)(i & 1), 0};
          } else if (shape == 2) {   /* every key's home is the table's last
                                        slot: one dense run that wraps */
            do v++; while (copr::in_set_hash(v, (uint32_t)m) != m);
            it = InItem{v, (uint8_t)pu, 0};
          } else if (shape == 3) {   /* every item unmatchable but the last */
            it = InItem{i + 1 == n ? 5 : (1ull << 63) + i, (uint8_t)!pu, 0};
          } else {                   /* 0, 1, 2 ...: empty moves past the keys */
            it = InItem{i, (uint8_t)(i & 1), 0};
          }
          items.push_back(it);
        }
        check_list(items, pu != 0);
      }
    }
  }
  printf("%lld checks, %lld mismatches\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
