/* Stand-alone check of tikv_amd/csrc/group_keys.h: the slot word,
 * the tuple hash / fingerprint / equality, and the probe loop run as a
 * sequential insert / lookup model over small tables. Built by
 * test_group_keys_cpu.py with the host compiler and
 * -fsanitize=address,undefined. */
#include <stdio.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "../tikv_amd/csrc/group_keys.h"

using namespace copr;

static int checks = 0, bad = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    checks++;                                                         \
    if (!(c)) {                                                       \
      bad++;                                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);              \
    }                                                                 \
  } while (0)

static GkTuple tup(int64_t a, bool an, int64_t b, bool bn, int64_t c = 0,
                   bool cn = false, int64_t d = 0, bool dn = false) {
  GkTuple t{};
  t.v[0] = an ? 0 : a; t.nul[0] = an;
  t.v[1] = bn ? 0 : b; t.nul[1] = bn;
  t.v[2] = cn ? 0 : c; t.nul[2] = cn;
  t.v[3] = dn ? 0 : d; t.nul[3] = dn;
  return t;
}

/* sequential model of the device dictionary: rows[] are the immutable inputs,
 * slots[] the table; hash_of lets a test force collisions */
struct Model {
  std::vector<GkTuple> rows;
  std::vector<uint64_t> slots;
  int k;
  uint64_t filled = 0;
  Model(uint32_t n_slots, int k_) : slots(n_slots, 0), k(k_) {}
  int64_t insert(const GkTuple &t) {
    const uint64_t row = rows.size();
    rows.push_back(t);
    bool claimed = false;
    int64_t s = gk_probe(
        t, k, row, (uint32_t)slots.size() - 1u,
        [&](uint32_t i) { return slots[i]; },
        [&](uint32_t i, uint64_t w) -> uint64_t {
          uint64_t old = slots[i];
          if (old == 0) slots[i] = w;
          return old;
        },
        [&](uint64_t rep) { return rows.at(rep); }, &claimed);
    if (claimed) filled++;
    return s;
  }
};

struct TupLess {
  bool operator()(const GkTuple &a, const GkTuple &b) const {
    for (int i = 0; i < COPR_GROUP_MAX_KEYS; i++) {
      if (a.nul[i] != b.nul[i]) return a.nul[i] < b.nul[i];
      if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    }
    return false;
  }
};

int main() {
  /* slot word round trip, the last legal row included */
  const uint64_t rows[] = {0, 1, 2, 255, 65535, 0x7FFFFFFFull, 0xFFFFFFFDull};
  const uint32_t fps[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 0x12345678u};
  for (uint64_t r : rows)
    for (uint32_t f : fps) {
      uint64_t w = gk_slot_pack(f, r);
      CHECK(w != 0);
      CHECK(gk_slot_fp(w) == f);
      CHECK(gk_slot_row(w) == r);
    }

  /* equality: NULL is not 0, per column */
  CHECK(gk_tuple_eq(tup(0, false, 0, true), tup(0, false, 0, true), 2));
  CHECK(!gk_tuple_eq(tup(0, false, 0, true), tup(0, false, 0, false), 2));
  CHECK(!gk_tuple_eq(tup(0, false, 0, true), tup(0, true, 0, false), 2));
  CHECK(!gk_tuple_eq(tup(0, true, 0, true), tup(0, true, 0, false), 2));
  CHECK(gk_tuple_eq(tup(0, true, 0, true), tup(0, true, 0, true), 2));
  CHECK(!gk_tuple_eq(tup(1, false, 2, false), tup(2, false, 1, false), 2));
  /* only the first k cells count */
  CHECK(gk_tuple_eq(tup(1, false, 2, false, 3), tup(1, false, 2, false, 4), 2));
  CHECK(!gk_tuple_eq(tup(1, false, 2, false, 3), tup(1, false, 2, false, 4), 3));
  CHECK(!gk_tuple_eq(tup(1, false, 2, false, 3, false, 0, true),
                     tup(1, false, 2, false, 3, false, 0, false), 4));
  /* the hash separates what equality separates in the usual suspects */
  CHECK(gk_tuple_hash(tup(1, false, 2, false), 2) !=
        gk_tuple_hash(tup(2, false, 1, false), 2));
  CHECK(gk_tuple_hash(tup(0, false, 0, true), 2) !=
        gk_tuple_hash(tup(0, true, 0, false), 2));
  CHECK(gk_tuple_hash(tup(0, false, 0, true), 2) !=
        gk_tuple_hash(tup(0, false, 0, false), 2));
  CHECK(gk_tuple_hash(tup(0, true, 0, true), 2) !=
        gk_tuple_hash(tup(0, false, 0, false), 2));
  /* equal tuples hash alike whatever a NULL cell's value word holds */
  {
    GkTuple a = tup(5, false, 0, true), b = a;
    b.v[1] = 77;
    CHECK(gk_tuple_hash(a, 2) == gk_tuple_hash(b, 2));
    CHECK(gk_tuple_eq(a, b, 2));
  }

  /* insert / lookup model against std::map, tables of 8..256 slots, up to
     full: every tuple keeps one slot, distinct tuples get distinct slots */
  const int64_t ext[] = {INT64_MIN, -1, 0, 1, INT64_MAX};
  for (uint32_t n_slots = 8; n_slots <= 256; n_slots *= 2) {
    Model m(n_slots, 2);
    std::map<GkTuple, int64_t, TupLess> ref;
    uint64_t x = 88172645463325252ull + n_slots;
    bool saw_full = false;
    for (int it = 0; it < 2000; it++) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      const bool an = (x >> 8) % 7 == 0, bn = (x >> 16) % 5 == 0;
      GkTuple t = tup(ext[(x >> 24) % 5], an, (int64_t)((x >> 32) % 23), bn);
      int64_t s = m.insert(t);
      auto f = ref.find(t);
      if (f != ref.end()) {
        CHECK(s == f->second);
      } else if (s < 0) {
        /* full: only when every slot is taken */
        saw_full = true;
        CHECK(m.filled == n_slots);
      } else {
        for (auto &kv : ref) CHECK(kv.second != s);
        ref[t] = s;
        CHECK(s >= 0 && (uint32_t)s < n_slots);
      }
    }
    CHECK(m.filled == ref.size());
    if (n_slots <= 64) CHECK(saw_full);
  }

  /* wrap-around: a tuple whose home is the last slot, already taken, lands
     in slot 0 */
  {
    const uint32_t n_slots = 8;
    Model m(n_slots, 2);
    std::vector<GkTuple> last;
    for (int64_t a = 0; last.size() < 2 && a < 100000; a++) {
      GkTuple t = tup(a, false, 7, false);
      if (gk_hash_slot(gk_tuple_hash(t, 2), n_slots - 1) == n_slots - 1)
        last.push_back(t);
    }
    CHECK(last.size() == 2);
    CHECK(m.insert(last[0]) == (int64_t)n_slots - 1);
    CHECK(m.insert(last[1]) == 0);
    CHECK(m.insert(last[0]) == (int64_t)n_slots - 1);
    CHECK(m.insert(last[1]) == 0);
  }

  /* equal fingerprints, different tuples: a 32-bit collision is too rare to
     search for, so plant one: tuple a sits as row 0 in b's home slot under
     b's fingerprint. b must compare the tuples, move on and claim another
     slot. */
  {
    const uint32_t n_slots = 4;
    Model m(n_slots, 2);
    GkTuple a = tup(1, false, 2, false), b = tup(2, false, 1, false);
    const uint64_t hb = gk_tuple_hash(b, 2);
    /* plant a as row 0 under b's fingerprint in b's home slot */
    m.rows.push_back(a);
    m.slots[gk_hash_slot(hb, n_slots - 1)] = gk_slot_pack(gk_hash_fp(hb), 0);
    m.filled = 1;
    int64_t sb = m.insert(b);
    CHECK(sb >= 0);
    CHECK((uint32_t)sb != gk_hash_slot(hb, n_slots - 1));
    CHECK(gk_slot_row(m.slots[sb]) == 1);
    CHECK(m.insert(b) == sb);
  }

  /* full flag on a table of one slot */
  {
    Model m(1, 2);
    CHECK(m.insert(tup(1, false, 1, false)) == 0);
    CHECK(m.insert(tup(1, false, 1, false)) == 0);
    CHECK(m.insert(tup(1, false, 2, false)) == -1);
  }

  printf("%d checks, %d mismatches\n", checks, bad);
  return bad ? 1 : 0;
}
