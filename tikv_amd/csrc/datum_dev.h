/* datum_dev.h — device-side readers of the stored row bytes shared by the HIP
 * translation units: varints, one v1 datum (CellView / d_parse_datum), the
 * scaled decimal fast paths, a row-v2 int cell and the chunk lookup of the
 * TypeChunk encoders. Moved verbatim out of kernels.hip so that
 * chunk_var.hip reads rows with the very code the scan kernels use. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copr {

/* unaligned 8-byte little-endian window at an LDS byte pointer, built from
 * three ALIGNED ds_read_b32 (an unaligned ds_read_b64 replays at 64 cyc —
 * MI355X_MICROARCH §LDS / G17) */
__device__ static inline uint64_t lds_win8(const uint8_t *p) {
  uintptr_t up = (uintptr_t)p;
  /* two ALIGNED ds_read_b64 (2 cyc each); an unaligned b64 replays at 64 cyc
     and hipcc merges adjacent u32 reads into exactly that (G17) */
  const uint64_t *q = (const uint64_t *)(up & ~(uintptr_t)7);
  uint32_t sh = (uint32_t)(up & 7) * 8u;
  uint64_t lo = q[0];
  uint64_t hi = q[1];
  return sh ? ((lo >> sh) | (hi << (64 - sh))) : lo;
}

/* ---------------- row-v1 parse from LDS ----------------
 * datum split lengths per flag: datum.rs:1117-1155; varint: number.rs:445-520 */
__device__ static inline bool d_var_u64_slow(const uint8_t *p, uint32_t rem,
                                             uint64_t *v, uint32_t *n) {
  uint64_t val = 0;
  uint32_t i = 0;
  int shift = 0;
  while (i < rem && i < 9u) {
    uint64_t b = p[i];
    val |= (b & 0x7f) << shift;
    i++;
    if (b < 0x80) { *v = val; *n = i; return true; }
    shift += 7;
  }
  if (i == 9u && i < rem) {       /* 10th byte contributes 1 bit */
    val |= (uint64_t)(p[9] & 0x01) << 63;
    *v = val; *n = 10; return true;
  }
  return false;
}

__device__ static inline bool d_var_u64(const uint8_t *p, uint32_t rem,
                                        uint64_t *v, uint32_t *n) {
  /* branchless window path for <=8-byte varints (the byte-at-a-time loop
     costs ~6 divergent instructions per byte; this is ~20 uniform ones).
     The 8-byte LDS window may read past the varint inside the staged slab
     (slabs carry >=16 B slack). */
  if (rem >= 8) {
    uint64_t m = lds_win8(p);
    uint64_t stops = ~m & 0x8080808080808080ull;
    if (stops) {
      /* stop at byte k sets bit 8k+7; __ffsll is 1-based -> 8k+8; >>3 = k+1
         = the varint's byte count */
      uint32_t nb = (uint32_t)__ffsll((long long)stops) >> 3;   /* 1..8 */
      uint64_t val = (m & 0x7f) | ((m >> 8) & 0x7f) << 7 |
                     ((m >> 16) & 0x7f) << 14 | ((m >> 24) & 0x7f) << 21 |
                     ((m >> 32) & 0x7f) << 28 | ((m >> 40) & 0x7f) << 35 |
                     ((m >> 48) & 0x7f) << 42 | ((m >> 56) & 0x7f) << 49;
      val &= (1ull << (7u * nb)) - 1ull;      /* 7*8=56 < 64 */
      *v = val;
      *n = nb;
      return true;
    }
    /* 9-10-byte varints: rare, take the loop */
  }
  return d_var_u64_slow(p, rem, v, n);
}
__device__ static inline bool d_var_i64(const uint8_t *p, uint32_t rem,
                                        int64_t *v, uint32_t *n) {
  uint64_t uv;
  if (!d_var_u64(p, rem, &uv, n)) return false;
  uint64_t half = uv >> 1;
  *v = (uv & 1) ? (int64_t)~half : (int64_t)half;
  return true;
}
__device__ static inline uint64_t d_be_u64(const uint8_t *p) {
  uint64_t v = 0;
  #pragma unroll
  for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
  return v;
}

/* decimal payload -> scaled int (prec<=18); mirrors read_decimal
 * (decimal.rs:2204-2289) restricted to the scaled-i64 fast path. */
__device__ static const uint32_t TEN_POW_D[10] = {1,10,100,1000,10000,100000,
  1000000,10000000,100000000,1000000000};
__device__ static const uint8_t DIG2B[10] = {0,1,1,2,2,3,3,4,4,4};

__device__ static inline uint32_t d_decimal_scaled(const uint8_t *p, uint32_t rem,
                                                   int64_t *scaled, int32_t *frac) {
  if (rem < 3) return 0;
  uint32_t prec = p[0], fr = p[1];
  if (prec < fr || prec > 18) return 0;
  uint32_t int_cnt = prec - fr;
  uint32_t iw = int_cnt / 9, ld = int_cnt - iw * 9;
  uint32_t fw = fr / 9, td = fr - fw * 9;
  uint32_t need = 2 + iw * 4 + DIG2B[ld] + fw * 4 + DIG2B[td];
  if (rem < need) return 0;
  /* payload <= 16 bytes (prec <= 18): two 8-byte windows, fields extracted
     by shifts — the byte-pointer walk serialized the groups and its
     per-width switch diverged lanes with differing digit counts (decimal
     parse was ~1/3 of the cfg3 kernel, profiles/r04_cfg3_attribution) */
  uint64_t w0 = lds_win8(p + 2);
  uint64_t w1 = lds_win8(p + 10);
  uint32_t mask = (uint32_t)(w0 & 0x80) ? 0u : 0xFFFFFFFFu;
  w0 ^= 0x80ull;                          /* flip the first payload byte */
  bool neg = mask != 0;
  uint64_t acc = 0;
  uint32_t off = 0;
  auto field = [&](uint32_t z) -> uint32_t {
    uint32_t v = 0;
    #pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      if (j < z) {
        uint32_t bo = off + j;
        uint32_t b = bo < 8 ? (uint32_t)(w0 >> (8 * bo))
                            : (uint32_t)(w1 >> (8 * (bo - 8)));
        v = (v << 8) | (b & 0xFFu);
      }
    }
    off += z;
    int32_t sx = (int32_t)(v << (8 * (4 - z)));  /* sign-extend field */
    sx >>= 8 * (4 - z);
    return (uint32_t)sx ^ mask;
  };
  if (ld) {
    uint32_t w = field(DIG2B[ld]);
    if (w >= TEN_POW_D[ld]) return 0;   /* leading group: < 10^ld digits */
    acc = w;
  }
  for (uint32_t k = 0; k < iw; k++) {
    uint32_t w = field(4);
    if (w > 999999999u) return 0;
    acc = acc * 1000000000ull + w;
  }
  for (uint32_t k = 0; k < fw; k++) {
    uint32_t w = field(4);
    if (w > 999999999u) return 0;
    acc = acc * 1000000000ull + w;
  }
  if (td) {
    uint32_t w = field(DIG2B[td]);
    if (w >= TEN_POW_D[td]) return 0;
    acc = acc * TEN_POW_D[td] + w;
  }
  *scaled = neg ? -(int64_t)acc : (int64_t)acc;
  *frac = (int32_t)fr;
  return need;
}

/* wide decimal payload -> scaled i128 (prec <= 38); the same read_decimal
 * restatement as d_decimal_scaled with 128-bit accumulation
 * (decimal.rs:2204-2289). Returns consumed bytes, 0 = malformed/too wide. */
__device__ static inline uint32_t d_decimal_scaled128(const uint8_t *p,
                                                      uint32_t rem,
                                                      __int128 *scaled,
                                                      int32_t *frac) {
  if (rem < 3) return 0;
  uint32_t prec = p[0], fr = p[1];
  if (prec < fr || prec > 38) return 0;
  uint32_t int_cnt = prec - fr;
  uint32_t iw = int_cnt / 9, ld = int_cnt - iw * 9;
  uint32_t fw = fr / 9, td = fr - fw * 9;
  uint32_t need = 2 + iw * 4 + DIG2B[ld] + fw * 4 + DIG2B[td];
  if (rem < need) return 0;
  const uint8_t *q = p + 2;
  uint32_t mask = (q[0] & 0x80) ? 0u : 0xFFFFFFFFu;
  bool neg = mask != 0;
  bool first = true;
  unsigned __int128 acc = 0;
  auto rd_word = [&](uint32_t size) -> uint32_t {
    uint8_t b0 = q[0];
    if (first) { b0 ^= 0x80; first = false; }
    uint32_t r;
    switch (size) {
      case 1: r = (uint32_t)(int32_t)(int8_t)b0; break;
      case 2: r = (uint32_t)(((int32_t)(int8_t)b0 << 8) + (int32_t)q[1]); break;
      case 3: r = (b0 & 128) ? ((255u << 24) | ((uint32_t)b0 << 16) |
                                ((uint32_t)q[1] << 8) | q[2])
                             : (((uint32_t)b0 << 16) | ((uint32_t)q[1] << 8) | q[2]);
              break;
      default: r = (uint32_t)(((int32_t)(int8_t)b0 << 24) + ((int32_t)q[1] << 16) +
                              ((int32_t)q[2] << 8) + (int32_t)q[3]); break;
    }
    q += size;
    return r;
  };
  if (ld) {
    uint32_t w = rd_word(DIG2B[ld]) ^ mask;
    if (w >= TEN_POW_D[ld]) return 0;
    acc = w;
  }
  for (uint32_t k = 0; k < iw; k++) {
    uint32_t w = rd_word(4) ^ mask;
    if (w > 999999999u) return 0;
    acc = acc * 1000000000u + w;
  }
  for (uint32_t k = 0; k < fw; k++) {
    uint32_t w = rd_word(4) ^ mask;
    if (w > 999999999u) return 0;
    acc = acc * 1000000000u + w;
  }
  if (td) {
    uint32_t w = rd_word(DIG2B[td]) ^ mask;
    if (w >= TEN_POW_D[td]) return 0;
    acc = acc * TEN_POW_D[td] + w;
  }
  *scaled = neg ? -(__int128)acc : (__int128)acc;
  *frac = (int32_t)fr;
  return need;
}

/* one datum (flag+payload) view */
struct CellView {
  uint32_t len;        /* full datum length incl flag; 0 = error */
  uint8_t flag;
  bool is_null;
  bool has_int;
  int64_t ival;        /* also carries f64 BITS when has_real */
  bool has_real;
  bool has_dec;
  int64_t dscaled; int32_t dfrac;
  /* wide decimal (19..38 digits): payload pointer for a deferred
     d_decimal_scaled128 parse at the contribute site; null otherwise */
  const uint8_t *dwide;
  uint32_t dwide_rem;
};

__device__ static inline void d_parse_datum(const uint8_t *p, uint32_t rem, CellView *cv) {
  cv->len = 0; cv->is_null = false; cv->has_int = false; cv->has_dec = false;
  cv->has_real = false; cv->dwide = nullptr;
  if (rem == 0) return;
  uint8_t flag = p[0];
  cv->flag = flag;
  const uint8_t *pl = p + 1;
  uint32_t prem = rem - 1;
  switch (flag) {
    case 0:  /* NIL */
      cv->is_null = true; cv->len = 1; return;
    case 3:  /* INT: BE ^ sign */
      if (prem < 8) return;
      cv->has_int = true;
      cv->ival = (int64_t)(d_be_u64(pl) ^ 0x8000000000000000ull);
      cv->len = 9; return;
    case 4:  /* UINT: BE */
      if (prem < 8) return;
      cv->has_int = true;
      cv->ival = (int64_t)d_be_u64(pl);
      cv->len = 9; return;
    case 5: {  /* FLOAT: comparable f64 (convert.rs:16-22) -> raw bits */
      if (prem < 8) return;
      uint64_t u = d_be_u64(pl);
      if (u & 0x8000000000000000ull) u &= 0x7FFFFFFFFFFFFFFFull;
      else u = ~u;
      cv->has_real = true;
      cv->ival = (int64_t)u;
      cv->len = 9; return;
    }
    case 7:  /* DURATION: 8B */
      if (prem < 8) return;
      cv->len = 9; return;
    case 8: {  /* VAR_INT */
      int64_t v; uint32_t n;
      if (!d_var_i64(pl, prem, &v, &n)) return;
      cv->has_int = true; cv->ival = v; cv->len = 1 + n; return;
    }
    case 9: {  /* VAR_UINT */
      uint64_t v; uint32_t n;
      if (!d_var_u64(pl, prem, &v, &n)) return;
      cv->has_int = true; cv->ival = (int64_t)v; cv->len = 1 + n; return;
    }
    case 2: {  /* COMPACT_BYTES: varint len + raw */
      int64_t l; uint32_t n;
      if (!d_var_i64(pl, prem, &l, &n)) return;
      if (l < 0 || n + (uint64_t)l > prem) return;
      cv->len = 1 + n + (uint32_t)l; return;
    }
    case 1: {  /* BYTES: 9-byte groups until marker != 0xFF */
      uint32_t pos = 0;
      for (;;) {
        if (pos + 9 > prem) return;
        uint8_t marker = pl[pos + 8];
        pos += 9;
        if (marker != 0xFF) {
          if (0xFF - marker > 8) return;
          break;
        }
      }
      cv->len = 1 + pos; return;
    }
    case 6: {  /* DECIMAL */
      int64_t sc; int32_t fr;
      uint32_t n = d_decimal_scaled(pl, prem, &sc, &fr);
      if (!n) {
        if (prem < 2) return;
        uint32_t prec = pl[0], frc = pl[1];
        if (prec < frc) return;
        uint32_t int_cnt = prec - frc;
        uint32_t iw = int_cnt / 9, ldg = int_cnt - iw * 9;
        uint32_t fwc = frc / 9, tdg = frc - fwc * 9;
        uint32_t need = 2 + iw * 4 + DIG2B[ldg] + fwc * 4 + DIG2B[tdg];
        if (prem < need) return;
        /* 19..38-digit decimals: defer the 128-bit parse to the
           contribute site (sums), keep the walk moving */
        if (prec <= 38) { cv->dwide = pl; cv->dwide_rem = prem; }
        cv->len = 1 + need; return;
      }
      cv->has_dec = true; cv->dscaled = sc; cv->dfrac = fr;
      cv->len = 1 + n; return;
    }
    default:
      return;  /* JSON/VECTOR unsupported */
  }
}

/* v2 int cell: little-endian 1/2/4/8 bytes, signed sign-extends
 * (compat_v1.rs:12-38) */
__device__ static inline bool d_v2_int(const uint8_t *c, uint32_t n, bool uns,
                                       int64_t *v) {
  uint64_t u = 0;
  switch (n) {
    case 1: u = c[0]; if (!uns) u = (uint64_t)(int64_t)(int8_t)c[0]; break;
    case 2: u = (uint32_t)c[0] | ((uint32_t)c[1] << 8);
            if (!uns) u = (uint64_t)(int64_t)(int16_t)u; break;
    case 4: u = (uint32_t)c[0] | ((uint32_t)c[1] << 8) |
                ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            if (!uns) u = (uint64_t)(int64_t)(int32_t)u; break;
    case 8:
      #pragma unroll
      for (int b = 0; b < 8; b++) u |= (uint64_t)c[b] << (8 * b);
      break;
    default: return false;
  }
  *v = (int64_t)u;
  return true;
}

__device__ static inline uint32_t d_chunk_of(
    const uint64_t *__restrict__ prefix, uint32_t n_chunks, uint64_t pos) {
  uint32_t lo = 0, hi = n_chunks;
  while (lo + 1 < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (prefix[mid] <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace copr
