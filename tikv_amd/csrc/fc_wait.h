/* fc_wait.h — the host's end of the filter+count hand-over: the
 * wait on the sequence word the finalizing block stores last, and the
 * conversion of the kernel's wall-clock ticks. Pure C++: no HIP, no other
 * project header, so both compile and test on their own. */
#ifndef COPR_FC_WAIT_H
#define COPR_FC_WAIT_H

#include <stdint.h>
#include <chrono>

namespace copr {

/* the three pinned host words of a request, in the order the device stores
   them: count and ticks first, the sequence number behind a system-scope
   fence of its own */
enum { FCW_COUNT = 0, FCW_TICKS = 1, FCW_SEQ = 2, FCW_WORDS = 3 };

enum FcWait { FCW_ARRIVED = 0, FCW_EXPIRED = 1 };

/* Spins until words[FCW_SEQ] == expected (acquire: the count and ticks words
   read afterwards are the ones stored before it) or deadline_us of the steady
   clock have passed since the call. The clock is read once at entry and then
   every 256 spins (FCW_SPINS), so "expired" comes no later than one batch of
   spins and one look at the clock past the deadline.
   deadline_us 0 = expired at once, without a look at the word or the clock:
   the caller's fallback then does all the waiting. Any other value of the
   word, a stale sequence number included, is no arrival. */
enum { FCW_SPINS = 256 };

inline FcWait wait_seq(const volatile uint64_t *words, uint64_t expected,
                       uint64_t deadline_us) {
  if (!deadline_us) return FCW_EXPIRED;
  const uint64_t *seq = (const uint64_t *)&words[FCW_SEQ];
  const auto end = std::chrono::steady_clock::now() +
                   std::chrono::microseconds(deadline_us);
  for (;;) {
    for (int i = 0; i < FCW_SPINS; i++) {
      if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == expected)
        return FCW_ARRIVED;
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#endif
    }
    if (std::chrono::steady_clock::now() >= end) return FCW_EXPIRED;
  }
}

/* ticks of a clock running at rate_khz -> nanoseconds, rounded down:
   ticks x 10^6 / rate_khz without the product overflowing. 0 for 0 ticks and
   for an unknown rate (0); a result past 64 bits saturates. */
inline uint64_t ticks_to_ns(uint64_t ticks, uint32_t rate_khz) {
  if (!rate_khz) return 0;
  const uint64_t M = 1000000ull;
  const uint64_t q = ticks / rate_khz, r = ticks % rate_khz;
  if (q > UINT64_MAX / M) return UINT64_MAX;
  /* r < rate_khz < 2^32, so r x 10^6 < 2^52; frac < 10^6 */
  const uint64_t frac = r * M / rate_khz;
  const uint64_t whole = q * M;
  return whole > UINT64_MAX - frac ? UINT64_MAX : whole + frac;
}

}  // namespace copr
#endif
