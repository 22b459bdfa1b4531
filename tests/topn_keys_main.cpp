/* Stand-alone check of tikv_amd/csrc/topn_keys.h: the order
 * key transform against the reference comparator, its inverse, and the
 * candidate-cut rule against a linear scan. Built and run by
 * tests/test_topn_keys_cpu.py with -fsanitize=address,undefined. */
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "../tikv_amd/csrc/topn_keys.h"

using namespace copr;

struct Val { int64_t v; bool null; };

/* oracle/orc_exec.cpp's per-key comparison: <0 a first, 0 tie, >0 b first */
static int ref_cmp(const Val &a, const Val &b, bool uns, bool desc) {
  int c;
  if (a.null != b.null) c = a.null ? -1 : 1;          /* NULL first */
  else if (a.null) c = 0;
  else if (uns) {
    uint64_t ua = (uint64_t)a.v, ub = (uint64_t)b.v;
    c = ua < ub ? -1 : (ua > ub ? 1 : 0);
  } else {
    c = a.v < b.v ? -1 : (a.v > b.v ? 1 : 0);
  }
  return desc ? -c : c;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {                                  /* splitmix64 */
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  unsigned long long checks = 0, bad = 0;

  std::vector<Val> vals;
  vals.push_back({0, true});
  const uint64_t fixed[] = {
      0x8000000000000000ull /* INT64_MIN, 2^63 unsigned */,
      0x8000000000000001ull, 0x8000000000000005ull, 0xFFFFFFFFFFFFFFFFull /* -1 */,
      0xFFFFFFFFFFFFFFFEull, 0ull, 1ull, 2ull, 0x7FFFFFFFFFFFFFFFull /* INT64_MAX */,
      0x7FFFFFFFFFFFFFFEull, 0x00000000FFFFFFFFull, 0xFFFFFFFF00000000ull};
  for (uint64_t f : fixed) vals.push_back({(int64_t)f, false});
  for (int i = 0; i < 300; i++) {
    uint64_t r = rng();
    if (i % 3 == 0) r >>= (rng() % 64);                  /* small magnitudes */
    if (i % 7 == 0) r = ~r;
    vals.push_back({(int64_t)r, false});
  }

  for (int uns = 0; uns < 2; uns++)
    for (int desc = 0; desc < 2; desc++) {
      std::vector<uint8_t> rk(vals.size());
      std::vector<unsigned long long> u(vals.size());
      for (size_t i = 0; i < vals.size(); i++) {
        topn_key_encode(vals[i].v, vals[i].null, uns, desc, &rk[i], &u[i]);
        int64_t back;
        bool nul;
        topn_key_decode(rk[i], u[i], uns, desc, &back, &nul);
        checks++;
        if (nul != vals[i].null || (!nul && back != vals[i].v) || rk[i] > 1) bad++;
      }
      for (size_t a = 0; a < vals.size(); a++)
        for (size_t b = 0; b < vals.size(); b++) {
          int c = ref_cmp(vals[a], vals[b], uns, desc);
          bool lt = rk[a] != rk[b] ? rk[a] < rk[b] : u[a] < u[b];
          bool eq = rk[a] == rk[b] && u[a] == u[b];
          bool le = topn_comp_le(rk[a], u[a], rk[b], u[b]);
          checks++;
          if (lt != (c < 0) || eq != (c == 0) || le != (c <= 0)) bad++;
        }
    }

  /* cut rule: sorted composites + take -> c, against a linear scan */
  auto check_cut = [&](std::vector<std::pair<uint8_t, unsigned long long>> comp) {
    std::sort(comp.begin(), comp.end());
    const uint64_t m = comp.size();
    std::vector<uint8_t> rk(m ? m : 1);
    std::vector<unsigned long long> u(m ? m : 1);
    for (uint64_t i = 0; i < m; i++) { rk[i] = comp[i].first; u[i] = comp[i].second; }
    /* element perm[i] of (prk, pu) is position i of the sorted order */
    std::vector<uint32_t> perm(m ? m : 1);
    std::vector<uint8_t> prk(m ? m : 1);
    std::vector<unsigned long long> pu(m ? m : 1);
    for (uint64_t i = 0; i < m; i++) perm[i] = (uint32_t)i;
    for (uint64_t i = m; i > 1; i--) std::swap(perm[i - 1], perm[rng() % i]);
    for (uint64_t i = 0; i < m; i++) { prk[perm[i]] = rk[i]; pu[perm[i]] = u[i]; }
    for (uint64_t take = 0; take <= m + 2; take++) {
      uint64_t want;
      if (take == 0) want = 0;
      else if (m <= take) want = m;
      else {
        want = 0;
        for (uint64_t i = 0; i < m; i++)
          if (comp[i] <= comp[take - 1]) want++;
      }
      uint64_t got = topn_cut(rk.data(), u.data(), nullptr, m, take);
      checks++;
      if (got != want) bad++;
      /* the same order reached through a permutation of shuffled arrays */
      uint64_t got_p = topn_cut(prk.data(), pu.data(), perm.data(), m, take);
      checks++;
      if (got_p != want) bad++;
      if (take && m > take && !(got >= take && got <= m)) bad++;
    }
  };
  check_cut({});
  check_cut({{1, 5}});
  for (int m = 1; m <= 40; m++) {
    std::vector<std::pair<uint8_t, unsigned long long>> all_eq, distinct, runs, nulls;
    for (int i = 0; i < m; i++) {
      all_eq.push_back({1, 77});
      distinct.push_back({1, (unsigned long long)(1000 - i)});
      runs.push_back({1, (unsigned long long)(i / 3)});
      nulls.push_back({(uint8_t)(i % 4 == 0 ? 0 : 1),
                       i % 4 == 0 ? 0ull : (unsigned long long)(i % 5)});
    }
    check_cut(all_eq);
    check_cut(distinct);
    check_cut(runs);
    check_cut(nulls);
  }
  for (int t = 0; t < 200; t++) {
    std::vector<std::pair<uint8_t, unsigned long long>> rnd;
    int m = 1 + (int)(rng() % 60);
    unsigned long long dom = 1 + rng() % 8;
    for (int i = 0; i < m; i++)
      rnd.push_back({(uint8_t)(rng() % 5 == 0 ? 0 : 1), rng() % dom});
    for (auto &p : rnd)
      if (p.first == 0) p.second = 0;
    check_cut(rnd);
  }

  printf("topn keys: %llu checks, %llu mismatches\n", checks, bad);
  return bad ? 1 : 0;
}
