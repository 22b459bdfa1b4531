/* Stand-alone check of the host end of the filter+count hand-over
 * (tikv_amd/csrc/fc_wait.h): wait_seq against a std::thread that
 * plays the device, and ticks_to_ns against 128-bit integer arithmetic.
 * Built and run by tests/test_fc_wait_cpu.py with the host compiler, once
 * with -fsanitize=address,undefined and once with -fsanitize=thread.
 * Exit 0 = every case agrees. */
#include <stdint.h>
#include <stdio.h>
#include <chrono>
#include <thread>

#include "../tikv_amd/csrc/fc_wait.h"

using namespace copr;
using Clock = std::chrono::steady_clock;

static unsigned long long bad = 0;
#define CHECK(c, ...)                                                        \
  do {                                                                       \
    if (!(c)) {                                                              \
      if (bad++ < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    }                                                                        \
  } while (0)

/* the pinned area, on a line of its own */
struct alignas(64) Area { volatile uint64_t w[FCW_WORDS]; };

static uint64_t count_of(uint64_t seq) { return seq * 0x9E3779B97F4A7C15ull; }
static uint64_t ticks_of(uint64_t seq) { return ~seq ^ (seq << 17); }

/* the device's three stores: count and ticks, then the number with release
   ordering (the kernel's system-scope fence) */
static void device_store(Area *a, uint64_t seq) {
  a->w[FCW_COUNT] = count_of(seq);
  a->w[FCW_TICKS] = ticks_of(seq);
  __atomic_store_n((uint64_t *)&a->w[FCW_SEQ], seq, __ATOMIC_RELEASE);
}

/* smallest step the steady clock shows, in ns */
static uint64_t clock_granularity_ns() {
  uint64_t best = UINT64_MAX;
  for (int i = 0; i < 200; i++) {
    const auto t0 = Clock::now();
    auto t1 = Clock::now();
    while (t1 == t0) t1 = Clock::now();
    const uint64_t d = (uint64_t)std::chrono::duration_cast<
        std::chrono::nanoseconds>(t1 - t0).count();
    if (d < best) best = d;
  }
  return best;
}

/* what one batch of FCW_SPINS spins costs in this program, sanitizer and all:
   the median of 65 batches of the same load and pause over a word that never
   matches. Timed here, not through wait_seq, so that a wait_seq which looked
   at the clock too rarely could not stretch its own allowance. */
static uint64_t spin_batch_ns() {
  Area a{};
  const uint64_t *seq = (const uint64_t *)&a.w[FCW_SEQ];
  uint64_t d[65];
  for (uint64_t &x : d) {
    const auto t0 = Clock::now();
    for (int i = 0; i < FCW_SPINS; i++) {
      if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == 1) bad++;
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#endif
    }
    x = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
        Clock::now() - t0).count();
  }
  for (int i = 1; i < 65; i++)                      /* insertion sort */
    for (int j = i; j > 0 && d[j] < d[j - 1]; j--) {
      const uint64_t t = d[j]; d[j] = d[j - 1]; d[j - 1] = t;
    }
  return d[32];
}

static void test_arrival() {
  Area a{};
  const uint64_t N = 4000;
  uint64_t go = 0;             /* host -> device: the request to answer */
  std::thread dev([&] {
    for (uint64_t seq = 1; seq <= N; seq++) {
      while (__atomic_load_n(&go, __ATOMIC_ACQUIRE) != seq) {}
      device_store(&a, seq);
    }
  });
  for (uint64_t seq = 1; seq <= N; seq++) {
    __atomic_store_n(&go, seq, __ATOMIC_RELEASE);
    /* a deadline the writer cannot miss short of a stalled machine */
    const FcWait r = wait_seq(a.w, seq, 30u * 1000u * 1000u);
    CHECK(r == FCW_ARRIVED, "seq %llu: expired", (unsigned long long)seq);
    if (r != FCW_ARRIVED) break;
    CHECK(a.w[FCW_COUNT] == count_of(seq) && a.w[FCW_TICKS] == ticks_of(seq),
          "seq %llu: stale count or ticks", (unsigned long long)seq);
  }
  /* let the writer out if the loop above broke off */
  __atomic_store_n(&go, N + 1, __ATOMIC_RELEASE);
  if (bad) { dev.detach(); return; }
  dev.join();
}

static void test_stale_and_absent(uint64_t gran_ns, uint64_t batch_ns) {
  /* wait_seq reads the clock at entry and after every batch of spins, so it
     returns within one batch and one look at the clock of its deadline. The
     allowance has no constant in it: two batches as timed above (the timed
     loop is a copy of wait_seq's, not the same instructions) and 16 steps of
     the clock for the four reads of it between t0 and the end. A scheduler can take the thread away across
     the deadline for longer than that, so each case runs nine times and the
     shortest run is held to the bound; every run is held to the deadline
     from below. */
  const uint64_t slack_ns = 2 * batch_ns + 16 * gran_ns;
  const uint64_t deadline_us = 3000;
  for (int stale = 0; stale < 2; stale++) {
    uint64_t least = UINT64_MAX;
    for (int rep = 0; rep < 9; rep++) {
      Area a{};
      const uint64_t expected = 77;
      /* stale: the number of the request before; absent: the zeroed area */
      if (stale) device_store(&a, expected - 1);
      const auto t0 = Clock::now();
      const FcWait r = wait_seq(a.w, expected, deadline_us);
      const uint64_t ns = (uint64_t)std::chrono::duration_cast<
          std::chrono::nanoseconds>(Clock::now() - t0).count();
      CHECK(r == FCW_EXPIRED, "stale %d: arrived", stale);
      CHECK(ns >= deadline_us * 1000, "stale %d: gave up after %llu ns", stale,
            (unsigned long long)ns);
      if (ns < least) least = ns;
    }
    printf("stale %d: shortest wait %llu ns, bound %llu ns\n", stale,
           (unsigned long long)least,
           (unsigned long long)(deadline_us * 1000 + slack_ns));
    CHECK(least <= deadline_us * 1000 + slack_ns,
          "stale %d: never under %llu ns", stale, (unsigned long long)least);
  }
  /* a writer that keeps storing the stale number is no arrival either */
  Area a{};
  int stop = 0;
  std::thread dev([&] {
    while (!__atomic_load_n(&stop, __ATOMIC_ACQUIRE)) device_store(&a, 76);
  });
  CHECK(wait_seq(a.w, 77, deadline_us) == FCW_EXPIRED, "stale writer: arrived");
  __atomic_store_n(&stop, 1, __ATOMIC_RELEASE);
  dev.join();
}

static void test_zero_deadline() {
  Area a{};
  CHECK(wait_seq(a.w, 5, 0) == FCW_EXPIRED, "deadline 0, no word: arrived");
  /* 0 hands every wait to the fallback, a word that is there included */
  device_store(&a, 5);
  CHECK(wait_seq(a.w, 5, 0) == FCW_EXPIRED, "deadline 0, word there: arrived");
  CHECK(wait_seq(a.w, 5, 1) == FCW_ARRIVED, "deadline 1, word there: expired");
}

static void test_ticks() {
  const uint32_t rates[] = {100000u, 1u, 3u, 99999u, 0xFFFFFFFFu};
  for (uint32_t rate : rates) {
    const uint64_t top = (1ull << 63) / rate;
    const uint64_t ticks[] = {0, 1, 2, rate - 1ull, rate, rate + 1ull, 3730,
                              top - 1, top, top + 1, UINT64_MAX / 1000000u,
                              UINT64_MAX / 1000000u + 1, UINT64_MAX};
    for (uint64_t t : ticks) {
      const unsigned __int128 exact = (unsigned __int128)t * 1000000u / rate;
      const uint64_t want = exact > (unsigned __int128)UINT64_MAX
                                ? UINT64_MAX : (uint64_t)exact;
      const uint64_t got = ticks_to_ns(t, rate);
      CHECK(got == want, "ticks %llu rate %u: %llu, want %llu",
            (unsigned long long)t, rate, (unsigned long long)got,
            (unsigned long long)want);
    }
    CHECK(ticks_to_ns(0, rate) == 0, "0 ticks at rate %u", rate);
  }
  CHECK(ticks_to_ns(12345, 0) == 0, "unknown rate");
  /* the device's rate: 100 MHz, 10 ns a tick */
  CHECK(ticks_to_ns(3730, 100000u) == 37300, "3730 ticks at 100 MHz");
}

int main() {
  const uint64_t gran = clock_granularity_ns();
  const uint64_t batch = spin_batch_ns();
  test_arrival();
  test_stale_and_absent(gran, batch);
  test_zero_deadline();
  test_ticks();
  printf("clock step %llu ns, spin batch %llu ns, %llu mismatches\n",
         (unsigned long long)gran, (unsigned long long)batch, bad);
  return bad ? 1 : 0;
}
