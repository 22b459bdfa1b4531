/* kernels.hip — MI355X (gfx950/CDNA4) kernels for the coprocessor hot path.
 *
 * Every kernel here is HBM-bandwidth-bound integer/byte work (no MFMA — see
 * DESIGN.md §4). The shared design center: a 256-thread workgroup stages the
 * contiguous byte range of its row tile into LDS with coalesced uint4 loads,
 * then each lane parses its row from LDS at random byte offsets. This turns
 * the reference's per-KV branchy varint walk
 * (table_scan_executor.rs:209-256 process_v1) into HBM-sequential traffic.
 *
 * The aggregation kernels are templated on the aggregate count so every
 * per-row state is register-resident (a dynamically indexed local array
 * spills to scratch: 528 B/lane and ~5x wall in the first build of this
 * kernel). The project kernel (row-returning scans) is separate and
 * scratch-tolerant — it is not the hot path.
 *
 * Wavefront = 64 (CDNA4); grid-stride over row tiles so a launch covers the
 * chip's 256 CUs across all 8 XCDs (consecutive tiles land on different
 * XCDs, block b -> XCD b%8).
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "copr_internal.h"

namespace copr {

#define THREADS 256u

/* ---------------- LDS staging ----------------
 * Copy [gbase, gbase+len) of src into lds (lds holds an aligned superset;
 * returns the intra-LDS shift of gbase). Coalesced uint4 loads on the
 * 16B-aligned floor. */
__device__ static inline uint32_t stage_tile(const uint8_t *__restrict__ src,
                                             uint64_t gbase, uint32_t len,
                                             uint8_t *lds) {
  uint64_t abase = gbase & ~15ull;
  uint32_t shift = (uint32_t)(gbase - abase);
  uint32_t total = (len + shift + 15u) & ~15u;
  const uint4 *gs = (const uint4 *)(src + abase);
  uint4 *ld = (uint4 *)lds;
  uint32_t n16 = total >> 4;
  /* batched: 8 UNCONDITIONAL independent loads per lane in the main body
     (a per-element bounds branch makes hipcc wait vmcnt(0) per element —
     cdna_hip_programming §6 trap (c)), then a simple tail loop */
  uint32_t per_round = blockDim.x * 8u;
  uint32_t base = 0;
  for (; base + per_round <= n16; base += per_round) {
    uint4 tmp[8];
    #pragma unroll
    for (int j = 0; j < 8; j++)
      tmp[j] = gs[base + threadIdx.x + (uint32_t)j * blockDim.x];
    #pragma unroll
    for (int j = 0; j < 8; j++)
      ld[base + threadIdx.x + (uint32_t)j * blockDim.x] = tmp[j];
  }
  for (uint32_t i = base + threadIdx.x; i < n16; i += blockDim.x)
    ld[i] = gs[i];
  __syncthreads();
  return shift;
}

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

#define ROW_FOREACH_BEGIN(vp, vlen)                                     \
  {                                                                     \
    uint32_t _pos = 0;                                                  \
    if (!((vlen) == 0 || ((vlen) == 1 && (vp)[0] == 0))) {              \
      while (_pos < (vlen)) {                                           \
        if ((vp)[_pos] != 8) { parse_ok = false; break; }               \
        _pos++;                                                         \
        int64_t _cid; uint32_t _n;                                      \
        if (!d_var_i64((vp) + _pos, (vlen) - _pos, &_cid, &_n)) {       \
          parse_ok = false; break; }                                    \
        _pos += _n;                                                     \
        CellView _cv;                                                   \
        d_parse_datum((vp) + _pos, (vlen) - _pos, &_cv);                \
        if (_cv.len == 0) { parse_ok = false; break; }                  \
        const uint32_t cell_off = _pos; (void)cell_off;                 \
        const int64_t cell_id = _cid; const CellView &cell = _cv;

#define ROW_FOREACH_END()                                               \
        _pos += _cv.len;                                                \
      }                                                                 \
    }                                                                   \
  }

/* advance one row-v1 cell. Fast word path for the dominant shape
 * [VAR_INT flag][1-byte col id][VAR_INT/VAR_UINT (<=5 B) or NIL datum]:
 * one unaligned 8-byte LDS window + ALU varint extraction. Everything else
 * falls back to the generic byte parser (identical semantics). */
__device__ static inline bool next_cell(const uint8_t *vp, uint32_t vlen,
                                        uint32_t *pos, int64_t *cid,
                                        uint32_t *cell_off, CellView *cv) {
  uint32_t p = *pos;
  if (p + 8 <= vlen) {
    uint64_t x = lds_win8(vp + p);
    if ((x & 0xFF) != 8) return false;   /* col id must be VAR_INT */
    uint32_t b1 = (uint32_t)(x >> 8) & 0xFF;
    if (b1 < 0x80) {
      uint32_t half = b1 >> 1;
      *cid = (b1 & 1) ? (int64_t)(~(uint64_t)half) : (int64_t)half;
      uint32_t dflag = (uint32_t)(x >> 16) & 0xFF;
      *cell_off = p + 2;
      if (dflag == 8 || dflag == 9) {
        uint64_t m = x >> 24;            /* 5 payload bytes in the window */
        uint64_t stops = ~m & 0x8080808080ull;
        if (stops) {
          uint32_t n = ((uint32_t)__ffsll((long long)stops)) >> 3;  /* 1..5 */
          uint64_t vm = m & ((n == 5) ? 0xFFFFFFFFFFull : ((1ull << (8 * n)) - 1));
          uint64_t uv = (vm & 0x7f) | ((vm >> 8) & 0x7f) << 7 |
                        ((vm >> 16) & 0x7f) << 14 | ((vm >> 24) & 0x7f) << 21 |
                        ((vm >> 32) & 0x7f) << 28;
          cv->is_null = false; cv->has_dec = false; cv->has_real = false;
          cv->has_int = true; cv->flag = (uint8_t)dflag;
          if (dflag == 8) {
            uint64_t h2 = uv >> 1;
            cv->ival = (uv & 1) ? (int64_t)~h2 : (int64_t)h2;
          } else {
            cv->ival = (int64_t)uv;
          }
          cv->len = 1 + n;
          *pos = p + 3 + n;
          return true;
        }
        /* varint needs >5 bytes: generic datum parse below */
      } else if (dflag == 0) {
        cv->is_null = true; cv->has_int = false; cv->has_dec = false;
        cv->has_real = false;
        cv->flag = 0; cv->len = 1;
        *pos = p + 3;
        return true;
      }
      d_parse_datum(vp + p + 2, vlen - (p + 2), cv);
      if (cv->len == 0) return false;
      *pos = p + 2 + cv->len;
      return true;
    }
  }
  /* generic: byte-wise col id + datum */
  if (vp[p] != 8) return false;
  p++;
  uint32_t n;
  if (!d_var_i64(vp + p, vlen - p, cid, &n)) return false;
  p += n;
  d_parse_datum(vp + p, vlen - p, cv);
  if (cv->len == 0) return false;
  *cell_off = p;
  *pos = p + cv->len;
  return true;
}


/* fold-aggregate transforms (kinds DAGG_MAX_INT..DAGG_BIT_XOR): map the
 * value into a u64 whose fold identity is 0 */
__device__ static inline unsigned long long d_fold_xform(int32_t kind,
                                                         int64_t v, bool uns) {
  unsigned long long b = (unsigned long long)v;
  if (kind == DAGG_MAX_REAL || kind == DAGG_MIN_REAL) {
    /* f64 bits -> order-preserving u64 (same map the comparable-f64 key
       encode uses, convert.rs:16-22) */
    b = (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    return kind == DAGG_MAX_REAL ? b : ~b;
  }
  if (!uns) b ^= 0x8000000000000000ull;       /* order-preserving bias */
  switch (kind) {
    case DAGG_MAX_INT: return b;
    case DAGG_MIN_INT: return ~b;
    case DAGG_BIT_AND: return ~(unsigned long long)v;
    case DAGG_BIT_XOR: return (unsigned long long)v;
    default:           return (unsigned long long)v;   /* BIT_OR */
  }
}
__device__ static inline bool d_is_fold(int32_t kind) {
  return kind >= DAGG_MAX_INT && kind <= DAGG_BIT_XOR;
}
__device__ static inline bool d_is_xor(int32_t kind) { return kind == DAGG_BIT_XOR; }


struct AggColView { bool found, null, has_dec; int64_t iv, dsc; int32_t dfr;
                    const uint8_t *dwide; uint32_t dwrem; };

/* ---------------- row v2 (codec/row/v2/row_slice.rs:76-168) ---------------- */
struct V2Row {
  bool big;
  uint32_t nn, nl;
  const uint8_t *ids, *nulls, *offs, *vals;
  uint32_t vbytes;
};

__device__ static inline bool d_v2_parse(const uint8_t *p, uint32_t len, V2Row *r) {
  if (len < 6 || p[0] != 128) return false;
  uint8_t flags = p[1];
  r->big = (flags & 1) != 0;
  bool ck = (flags & 2) != 0;
  r->nn = (uint32_t)p[2] | ((uint32_t)p[3] << 8);
  r->nl = (uint32_t)p[4] | ((uint32_t)p[5] << 8);
  uint32_t idw = r->big ? 4u : 1u, offw = r->big ? 4u : 2u;
  uint32_t pos = 6;
  if (pos + idw * (r->nn + r->nl) + offw * r->nn > len) return false;
  r->ids = p + pos; pos += idw * r->nn;
  r->nulls = p + pos; pos += idw * r->nl;
  r->offs = p + pos; pos += offw * r->nn;
  r->vals = p + pos;
  r->vbytes = len - pos;
  if (ck) {                        /* checksum trailer after the last value */
    uint32_t vend = 0;
    if (r->nn) {
      const uint8_t *o = r->offs + offw * (r->nn - 1);
      vend = r->big ? ((uint32_t)o[0] | ((uint32_t)o[1] << 8) |
                       ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24))
                    : ((uint32_t)o[0] | ((uint32_t)o[1] << 8));
    }
    if (vend > r->vbytes) return false;
    r->vbytes = vend;
  }
  return true;
}

/* search_in_non_null_ids / search_in_null_ids (row_slice.rs:125-196):
 * 1 = found (start,end set), 0 = in null list, -1 = absent */
__device__ static inline int d_v2_find(const V2Row &r, int64_t cid,
                                       uint32_t *s, uint32_t *e) {
  if (cid <= 0) return -1;
  if (!r.big && cid > 255) return -1;
  if (r.big && cid > 0xFFFFFFFFll) return -1;
  uint32_t target = (uint32_t)cid;
  uint32_t offw = r.big ? 4u : 2u;
  int lo = 0, hi = (int)r.nn - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    uint32_t v = r.big ? ((uint32_t)r.ids[4 * mid] | ((uint32_t)r.ids[4 * mid + 1] << 8) |
                          ((uint32_t)r.ids[4 * mid + 2] << 16) | ((uint32_t)r.ids[4 * mid + 3] << 24))
                       : r.ids[mid];
    if (v == target) {
      const uint8_t *o = r.offs + offw * mid;
      uint32_t end = r.big ? ((uint32_t)o[0] | ((uint32_t)o[1] << 8) |
                              ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24))
                           : ((uint32_t)o[0] | ((uint32_t)o[1] << 8));
      uint32_t st = 0;
      if (mid > 0) {
        const uint8_t *po = r.offs + offw * (mid - 1);
        st = r.big ? ((uint32_t)po[0] | ((uint32_t)po[1] << 8) |
                      ((uint32_t)po[2] << 16) | ((uint32_t)po[3] << 24))
                   : ((uint32_t)po[0] | ((uint32_t)po[1] << 8));
      }
      if (st > end || end > r.vbytes) return -1;
      *s = st; *e = end;
      return 1;
    }
    if (v < target) lo = mid + 1; else hi = mid - 1;
  }
  lo = 0; hi = (int)r.nl - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    uint32_t v = r.big ? ((uint32_t)r.nulls[4 * mid] | ((uint32_t)r.nulls[4 * mid + 1] << 8) |
                          ((uint32_t)r.nulls[4 * mid + 2] << 16) | ((uint32_t)r.nulls[4 * mid + 3] << 24))
                       : r.nulls[mid];
    if (v == target) return 0;
    if (v < target) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
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

template <int NAGGS, bool IS_HASH>
__device__ static inline bool d_v2_collect(const ScanPlan &plan,
                                           const uint8_t *vp, uint32_t vlen,
                                           bool *filt_found, bool *filt_null,
                                           int64_t *filt_v, bool *grp_found,
                                           bool *grp_null, int64_t *grp_v,
                                           AggColView (&cols)[NAGGS],
                                           bool parse_grp = true,
                                           bool *f2_found = nullptr,
                                           bool *f2_null = nullptr,
                                           int64_t *f2_v = nullptr) {
  V2Row r;
  if (!d_v2_parse(vp, vlen, &r)) return false;
  /* v2 Float/Double cells keep the v1 FLOAT payload (compat_v1.rs:68-72):
     8-byte BE comparable f64 -> IEEE bits for the real channels */
  auto v2_real_bits = [&](uint32_t s, uint32_t e, int64_t *out) -> bool {
    if (e - s != 8) return false;
    uint64_t u = d_be_u64(r.vals + s);
    *out = (int64_t)((u & 0x8000000000000000ull)
                         ? (u ^ 0x8000000000000000ull) : ~u);
    return true;
  };
  if (plan.has_filter) {
    uint32_t s, e;
    int st = d_v2_find(r, plan.filter_col_id, &s, &e);
    if (st >= 0) {
      *filt_found = true;
      if (st == 0) *filt_null = true;
      else if (plan.filter_is_real) {
        if (!v2_real_bits(s, e, filt_v)) return false;
      } else if (!d_v2_int(r.vals + s, e - s, plan.filter_col_unsigned, filt_v))
        return false;
    }
  }
  if (plan.filter2_on && f2_found) {
    uint32_t s, e;
    int st = d_v2_find(r, plan.filter2_col_id, &s, &e);
    if (st >= 0) {
      *f2_found = true;
      if (st == 0) *f2_null = true;
      else if (plan.filter2_is_real) {
        if (!v2_real_bits(s, e, f2_v)) return false;
      } else if (!d_v2_int(r.vals + s, e - s, plan.filter2_col_unsigned, f2_v))
        return false;
    }
  }
  if (IS_HASH && parse_grp) {
    uint32_t s, e;
    int st = d_v2_find(r, plan.group_col_id, &s, &e);
    if (st >= 0) {
      *grp_found = true;
      if (st == 0) *grp_null = true;
      else if (!d_v2_int(r.vals + s, e - s, plan.group_col_unsigned, grp_v))
        return false;
    }
  }
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) {
    const DevAggSpec &sp = plan.aggs[a];
    if (sp.kind == DAGG_COUNT_ROWS) continue;
    uint32_t s, e;
    int st = d_v2_find(r, sp.col_id, &s, &e);
    if (st < 0) continue;
    cols[a].found = true;
    if (st == 0) { cols[a].null = true; continue; }
    if (sp.kind == DAGG_SUM_DEC) {
      int64_t sc; int32_t fr;
      if (!d_decimal_scaled(r.vals + s, e - s, &sc, &fr)) return false;
      cols[a].has_dec = true; cols[a].dsc = sc; cols[a].dfr = fr;
    } else if (sp.kind == DAGG_SUM_REAL || sp.kind == DAGG_MAX_REAL ||
               sp.kind == DAGG_MIN_REAL) {
      /* v2 Float/Double cell keeps the v1 FLOAT datum payload verbatim
         (compat_v1.rs:68-72): 8-byte BE comparable f64 -> IEEE bits */
      if (e - s != 8) return false;
      uint64_t u = d_be_u64(r.vals + s);
      cols[a].iv = (int64_t)((u & 0x8000000000000000ull)
                                 ? (u ^ 0x8000000000000000ull) : ~u);
    } else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_XCAP ||
               d_is_fold(sp.kind)) {
      if (!d_v2_int(r.vals + s, e - s, sp.col_unsigned, &cols[a].iv)) return false;
    }
    /* COUNT_COL: found/null is all that matters */
  }
  return true;
}


/* IndexScan positional walk (index_scan_executor.rs:504-560 old-collation
 * local path): vp = the whole index KEY; comparable datums start at byte 19;
 * cell "ids" are positions 0..n-1, with the trailing int-handle datum at
 * position index_n_cols. */
/* Index VALUE layouts (index_scan_executor.rs:322-371,416-422,700-885):
 *   old (len <= 9): [8B BE handle]['flag'] for unique, or '0'/empty for
 *     non-unique;
 *   new (len > 9): TailLen | [VersionFlag Version] | Options | tail,
 *     options = [127 CHandle-len u16le CHandle] [126 pid 8B]
 *               [128... restore-data row-v2 to the segment end];
 *     handle = first 8 BE bytes of the tail when TailLen >= 8
 *     (decode_int_handle_from_value :416-422 on build_operations' tail).
 * Returns: 1 ok, 0 malformed. *restore/-len = V4 restore-data row (version
 * 0: columns must be read from this row-v2, :903-907); V5 restore data is
 * skipped (int columns are never restored — need_restored_data is false
 * for them, :639-698). Common-handle options are out of the int-handle
 * native subset -> malformed (loud). */
__device__ static inline bool d_index_value_split(const uint8_t *v, uint32_t n,
                                                  int64_t *handle, bool *has_handle,
                                                  const uint8_t **restore,
                                                  uint32_t *restore_len) {
  *has_handle = false;
  *restore = nullptr;
  *restore_len = 0;
  if (n <= 9) {                    /* old encoding (:336-345) */
    if (n >= 8) {
      *handle = (int64_t)d_be_u64(v);   /* plain BE u64, NOT comparable */
      *has_handle = true;
    }
    return true;                   /* '0' / empty / short: no handle */
  }
  uint32_t tail_len = v[0];
  if (tail_len >= n) return false;
  int version = 0;
  uint32_t opt = 1;
  if ((tail_len == 0 || tail_len == 1) && v[1] == 125 /*VERSION_FLAG*/) {
    version = v[2];
    opt = 3;
  }
  if (n < opt + tail_len) return false;
  uint32_t opt_end = n - tail_len;
  while (opt < opt_end) {
    uint8_t f = v[opt];
    if (f == 127) return false;          /* common handle: not int-handle */
    if (f == 126) {                      /* partition id segment */
      if (opt + 9 > opt_end) return false;
      opt += 9;
      continue;
    }
    if (f == 128) {                      /* restore data = row-v2 to end */
      if (version == 0) {
        *restore = v + opt;
        *restore_len = opt_end - opt;
      }                                  /* V5: ints never restored; skip */
      opt = opt_end;
      break;
    }
    return false;                        /* unknown segment */
  }
  if (tail_len >= 8) {
    *handle = (int64_t)d_be_u64(v + n - tail_len);
    *has_handle = true;
  }
  return true;
}

template <int NAGGS, bool IS_HASH>
__device__ static inline bool d_index_collect(const ScanPlan &plan,
                                              const uint8_t *vp, uint32_t vlen,
                                              uint64_t my_row,
                                              bool *filt_found, bool *filt_null,
                                              int64_t *filt_v, bool *grp_found,
                                              bool *grp_null, int64_t *grp_v,
                                              AggColView (&cols)[NAGGS],
                                              int64_t *handle_out,
                                              bool *handle_found) {
  if (vlen < 19 || vp[0] != 't' || vp[9] != '_' || vp[10] != 'i') return false;
  /* The VALUE decides the layout. New-format values (len > 9) can carry
     restore data that OVERRIDES the key columns, so they must be split
     before the key walk — but only regions that contain such values pay
     for it (aux_max_vlen > 9). Old-format regions read the value lazily,
     only for rows whose key carries no trailing handle. */
  int64_t vhandle = 0;
  bool v_has_handle = false;
  const uint8_t *restore = nullptr;
  uint32_t restore_len = 0;
  bool value_split_done = false;
  auto split_value = [&]() -> bool {
    uint64_t o0 = plan.aux_val_offs[my_row], o1 = plan.aux_val_offs[my_row + 1];
    value_split_done = true;
    return d_index_value_split(plan.aux_vals + o0, (uint32_t)(o1 - o0),
                               &vhandle, &v_has_handle, &restore,
                               &restore_len);
  };
  if (plan.aux_vals && plan.aux_max_vlen > 9) {
    if (!split_value()) return false;
  }
  *handle_found = false;

  /* per-cell consumer shared by the key walk and the restore-row path */
  auto match_cell = [&](int64_t cell_id, const CellView &cell) -> bool {
    if (cell_id == (int64_t)plan.index_n_cols) {   /* trailing handle datum */
      if (!cell.has_int) return false;
      *handle_out = cell.ival;
      *handle_found = true;
    }
    if (plan.has_filter && !*filt_found && cell_id == plan.filter_col_id) {
      *filt_found = true;
      if (cell.is_null) *filt_null = true;
      else if (cell.has_int) *filt_v = cell.ival;
      else return false;
    }
    if (IS_HASH && !*grp_found && cell_id == plan.group_col_id) {
      *grp_found = true;
      if (cell.is_null) *grp_null = true;
      else if (cell.has_int) *grp_v = cell.ival;
      else return false;
    }
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      if (plan.aggs[a].kind == DAGG_COUNT_ROWS || cols[a].found) continue;
      if (cell_id == plan.aggs[a].col_id) {
        cols[a].found = true;
        cols[a].null = cell.is_null;
        cols[a].iv = cell.ival;
        cols[a].has_dec = cell.has_dec;
        cols[a].dsc = cell.dscaled; cols[a].dfr = cell.dfrac;
        cols[a].dwide = cell.dwide; cols[a].dwrem = cell.dwide_rem;
        if (!cell.is_null && !cell.has_int && !cell.has_real &&
            !cell.has_dec && !cell.dwide)
          return false;
      }
    }
    return true;
  };

  if (restore) {
    /* V4 restore data: ALL index columns come from the restore row-v2,
       keyed by the reference column ids (extract_columns_from_row_format
       :483-501); the key datums are not consulted */
    V2Row r;
    if (!d_v2_parse(restore, restore_len, &r)) return false;
    for (int32_t p = 0; p < plan.index_n_cols; p++) {
      uint32_t s, e;
      int st = d_v2_find(r, plan.index_real_ids[p], &s, &e);
      if (st < 0) return false;          /* missing column (:496-497) */
      CellView cell{};
      if (st == 0) {
        cell.is_null = true;
      } else {
        /* int columns only in the native index subset; the consumer's
           signedness drives the v2 sign extension */
        int64_t iv;
        bool uns = false;
        if (plan.has_filter && p == plan.filter_col_id)
          uns = plan.filter_col_unsigned != 0;
        else if (IS_HASH && p == plan.group_col_id)
          uns = plan.group_col_unsigned != 0;
        else
          for (int a = 0; a < NAGGS; a++)
            if (plan.aggs[a].kind != DAGG_COUNT_ROWS &&
                p == plan.aggs[a].col_id) {
              uns = plan.aggs[a].col_unsigned != 0;
              break;
            }
        if (!d_v2_int(r.vals + s, e - s, uns, &iv)) return false;
        cell.has_int = true;
        cell.ival = iv;
      }
      if (!match_cell(p, cell)) return false;
    }
  } else {
    uint32_t pos = 19;
    int64_t ci = 0;
    while (pos < vlen) {
      CellView cell;
      d_parse_datum(vp + pos, vlen - pos, &cell);
      if (cell.len == 0) return false;
      if (!match_cell(ci, cell)) return false;
      pos += cell.len;
      ci++;
    }
  }

  if (!*handle_found) {
    if (!value_split_done && plan.aux_vals && !split_value()) return false;
    if (v_has_handle) {
      /* unique index: PK int handle lives in the value (:553-562) */
      CellView cell{};
      cell.has_int = true;
      cell.ival = vhandle;
      if (!match_cell((int64_t)plan.index_n_cols, cell)) return false;
    }
  }
  return true;
}

/* predicate eval (impl_compare.rs:66-160) */
__device__ static inline int d_cmp_int(int64_t l, int64_t r, bool lu, bool ru) {
  if (lu && ru) { uint64_t a = (uint64_t)l, b = (uint64_t)r; return a < b ? -1 : a > b ? 1 : 0; }
  if (!lu && !ru) return l < r ? -1 : l > r ? 1 : 0;
  if (lu && !ru) {
    if (r < 0 || (uint64_t)l > 0x7FFFFFFFFFFFFFFFull) return 1;
    return l < r ? -1 : l > r ? 1 : 0;
  }
  if (l < 0 || (uint64_t)r > 0x7FFFFFFFFFFFFFFFull) return -1;
  return l < r ? -1 : l > r ? 1 : 0;
}
__device__ static inline bool d_cmp_res(int32_t kind, int ord) {
  switch (kind) {
    case CMP_LT: return ord < 0;
    case CMP_LE: return ord <= 0;
    case CMP_GT: return ord > 0;
    case CMP_GE: return ord >= 0;
    case CMP_EQ: return ord == 0;
    default:     return ord != 0;
  }
}

/* Real comparer (impl_compare.rs:66-160 Real path): values travel as f64
 * BITS in the i64 channels; Real is guaranteed non-NaN in the reference
 * (Real::new rejects NaN), so plain f64 ordering is total */
__device__ static inline int d_cmp_real(int64_t lbits, int64_t rbits) {
  double l = __longlong_as_double((long long)lbits);
  double r = __longlong_as_double((long long)rbits);
  return l < r ? -1 : l > r ? 1 : 0;
}

/* evaluate the plan's filter for one row's decoded filter-column state */
__device__ static inline bool d_filter_keep(const ScanPlan &plan, bool found,
                                            bool is_null, int64_t v) {
  if (plan.filter_decode_only) return true;
  if (!plan.has_filter) return true;
  if (!found) {
    if (plan.filter_missing_null) is_null = true;
    else { v = plan.filter_missing_val; is_null = false; }
  }
  if (plan.filter_const_null || is_null) return false;
  return d_cmp_res(plan.filter_cmp,
                   plan.filter_is_real
                       ? d_cmp_real(v, plan.filter_const)
                       : d_cmp_int(v, plan.filter_const,
                                   plan.filter_col_unsigned,
                                   plan.filter_const_unsigned));
}


__device__ static inline bool d_filter2_keep(const ScanPlan &plan,
                                             bool found, bool is_null,
                                             int64_t v) {
  if (!plan.filter2_on) return true;
  if (!found) {
    if (plan.filter2_missing_null) is_null = true;
    else { v = plan.filter2_missing_val; is_null = false; }
  }
  if (plan.filter2_const_null || is_null) return false;
  return d_cmp_res(plan.filter2_cmp,
                   plan.filter2_is_real
                       ? d_cmp_real(v, plan.filter2_const)
                       : d_cmp_int(v, plan.filter2_const,
                                   plan.filter2_col_unsigned,
                                   plan.filter2_const_unsigned));
}

/* PLUS / MINUS / MULTIPLY in the IntInt / IntUint / UintInt / UintUint
 * variant the operands' UNSIGNED flags select (impl_arithmetic.rs): with an
 * unsigned operand the result is BIGINT UNSIGNED and must lie in
 * [0, 2^64-1]; a negative signed factor times an unsigned one is out of
 * range whatever the unsigned one is. Returns true on overflow. */
__device__ static inline bool d_arith_int(int32_t sig, int64_t a, int64_t b,
                                          bool lu, bool ru, int64_t *res) {
  if (!lu && !ru) {
    long long r;
    bool ovf =
        sig == COPR_SIG_PLUS_INT
            ? __builtin_add_overflow((long long)a, (long long)b, &r)
            : sig == COPR_SIG_MINUS_INT
                  ? __builtin_sub_overflow((long long)a, (long long)b, &r)
                  : __builtin_mul_overflow((long long)a, (long long)b, &r);
    *res = r;
    return ovf;
  }
  unsigned long long x = (unsigned long long)a, y = (unsigned long long)b, r;
  bool ovf;
  if (sig == COPR_SIG_PLUS_INT) {
    if (lu && ru) {
      ovf = __builtin_add_overflow(x, y, &r);
    } else {
      int64_t s = lu ? b : a;            /* the signed operand */
      unsigned long long u = lu ? x : y;
      ovf = s >= 0 ? __builtin_add_overflow(u, (unsigned long long)s, &r)
                   : __builtin_sub_overflow(u, 0 - (unsigned long long)s, &r);
    }
  } else if (sig == COPR_SIG_MINUS_INT) {
    if (lu && ru) ovf = __builtin_sub_overflow(x, y, &r);
    else if (ru) ovf = __builtin_sub_overflow(x, y, &r) || a < 0;
    else ovf = b >= 0 ? __builtin_sub_overflow(x, y, &r)
                      : __builtin_add_overflow(x, 0 - y, &r);
  } else {
    ovf = __builtin_mul_overflow(x, y, &r) || (!lu && a < 0) || (!ru && b < 0);
  }
  *res = (int64_t)r;
  return ovf;
}

/* evaluate the plan's RPN predicate over the captured columns: NULL-aware
 * logical ops (impl_op.rs), comparers and arithmetic in the variant the
 * operands' UNSIGNED flags select; overflow errors the request. A gate node
 * (kind 4) ends every condition of the selection but the last: a row whose
 * condition value is not true is dropped there and no later node sees it,
 * as selection_executor.rs:86 hands a later condition only the rows the
 * earlier ones kept.
 * Returns keep; *err set on overflow / malformed program. */
__device__ static inline bool d_rpn_keep(const ScanPlan &plan,
                                         bool f1_found, bool f1_null,
                                         int64_t f1_v, bool f2_found,
                                         bool f2_null, int64_t f2_v,
                                         bool *err,
                                         int64_t xv0 = 0, uint8_t xn0 = 0,
                                         int64_t xv1 = 0, uint8_t xn1 = 0) {
  int64_t sv[4];
  uint8_t sn[4], su[4];
  int sp = 0;
  /* missing-column fill, same as the fixed filter path */
  if (!f1_found) {
    if (plan.filter_missing_null) f1_null = true;
    else { f1_v = plan.filter_missing_val; f1_null = false; }
  }
  if (!f2_found) {
    if (plan.filter2_missing_null) f2_null = true;
    else { f2_v = plan.filter2_missing_val; f2_null = false; }
  }

  for (int i = 0; i < plan.rpn_n; i++) {
    const DevRpnNode &nd = plan.rpn[i];
    if (nd.kind == 0) {
      if (sp >= 4) { *err = true; return false; }
      if (nd.slot >= 2) {
        /* scalars, never an indexed array: a memory-addressable capture
           array spilled every instantiation of the callers */
        sv[sp] = nd.slot == 2 ? xv0 : xv1;
        sn[sp] = nd.slot == 2 ? xn0 : xn1;
      } else {
        sv[sp] = nd.slot ? f2_v : f1_v;
        sn[sp] = nd.slot ? (f2_null ? 1 : 0) : (f1_null ? 1 : 0);
      }
      su[sp] = (uint8_t)nd.uns;
      sp++;
    } else if (nd.kind == 1) {
      if (sp >= 4) { *err = true; return false; }
      sv[sp] = nd.cval; sn[sp] = 0; su[sp] = (uint8_t)nd.uns;
      sp++;
    } else if (nd.kind == 2) {
      if (sp >= 4) { *err = true; return false; }
      sv[sp] = 0; sn[sp] = 1; su[sp] = 0;
      sp++;
    } else if (nd.kind == 4) {
      if (sp != 1) { *err = true; return false; }
      if (sn[0] != 0 || sv[0] == 0) return false;
      sp = 0;
    } else {
      int na = (nd.sig == COPR_SIG_UNARY_NOT ||
                nd.sig == COPR_SIG_INT_IS_NULL ||
                nd.sig == COPR_SIG_INT_IS_TRUE ||
                nd.sig == COPR_SIG_INT_IS_FALSE) ? 1 : 2;
      if (sp < na) { *err = true; return false; }
      int b = sp - na;
      bool n0 = sn[b] != 0, n1 = na == 2 && sn[b + 1] != 0;
      int64_t a0 = sv[b], a1 = na == 2 ? sv[b + 1] : 0;
      int64_t rv = 0;
      uint8_t rn = 0;
      switch (nd.sig) {
        case COPR_SIG_LT_INT: case COPR_SIG_LE_INT: case COPR_SIG_GT_INT:
        case COPR_SIG_GE_INT: case COPR_SIG_EQ_INT: case COPR_SIG_NE_INT: {
          if (n0 || n1) { rn = 1; break; }
          int cmp = nd.sig == COPR_SIG_LT_INT ? CMP_LT :
                    nd.sig == COPR_SIG_LE_INT ? CMP_LE :
                    nd.sig == COPR_SIG_GT_INT ? CMP_GT :
                    nd.sig == COPR_SIG_GE_INT ? CMP_GE :
                    nd.sig == COPR_SIG_EQ_INT ? CMP_EQ : CMP_NE;
          rv = d_cmp_res(cmp, d_cmp_int(a0, a1, su[b], su[b + 1])) ? 1 : 0;
          break;
        }
        case COPR_SIG_LOGICAL_AND: {
          bool t0f = !n0 && a0 == 0, t1f = !n1 && a1 == 0;
          if (t0f || t1f) rv = 0;
          else if (n0 || n1) rn = 1;
          else rv = 1;
          break;
        }
        case COPR_SIG_LOGICAL_OR: {
          bool t0 = !n0 && a0 != 0, t1 = !n1 && a1 != 0;
          if (t0 || t1) rv = 1;
          else if (n0 || n1) rn = 1;
          else rv = 0;
          break;
        }
        case COPR_SIG_UNARY_NOT:
          if (n0) rn = 1;
          else rv = a0 == 0 ? 1 : 0;
          break;
        case COPR_SIG_PLUS_INT: case COPR_SIG_MINUS_INT:
        case COPR_SIG_MULTIPLY_INT: {
          if (n0 || n1) { rn = 1; break; }
          if (d_arith_int(nd.sig, a0, a1, su[b] != 0, su[b + 1] != 0, &rv)) {
            *err = true;
            return false;
          }
          break;
        }
        case COPR_SIG_INT_IS_NULL: rv = n0 ? 1 : 0; break;
        case COPR_SIG_INT_IS_TRUE: rv = (!n0 && a0 != 0) ? 1 : 0; break;
        case COPR_SIG_INT_IS_FALSE: rv = (!n0 && a0 == 0) ? 1 : 0; break;
        default: *err = true; return false;
      }
      sp = b;
      sv[sp] = rv; sn[sp] = rn; su[sp] = (uint8_t)nd.uns;
      sp++;
    }
  }
  if (sp != 1) { *err = true; return false; }
  return sn[0] == 0 && sv[0] != 0;   /* as_mysql_bool */
}

/* combined keep decision over the two capture channels */
__device__ static inline bool d_keep2(const ScanPlan &plan, bool f1_found,
                                      bool f1_null, int64_t f1_v,
                                      bool f2_found, bool f2_null,
                                      int64_t f2_v, bool *err,
                                      int64_t xv0 = 0, uint8_t xn0 = 0,
                                      int64_t xv1 = 0, uint8_t xn1 = 0) {
  if (plan.rpn_on)
    return d_rpn_keep(plan, f1_found, f1_null, f1_v, f2_found, f2_null, f2_v,
                      err, xv0, xn0, xv1, xn1);
  return d_filter_keep(plan, f1_found, f1_null, f1_v) &&
         d_filter2_keep(plan, f2_found, f2_null, f2_v);
}

/* pull the xcap channels (2..3) out of the capture slots with STATIC
 * indexing only (an indexed read of cols[] would force the whole per-lane
 * array to scratch) and apply the missing fill */
template <int NAGGS>
__device__ static inline void d_xcap_extract(const ScanPlan &plan,
                                             const AggColView (&cols)[NAGGS],
                                             int64_t *xv0, uint8_t *xn0,
                                             int64_t *xv1, uint8_t *xn1) {
  int64_t v0 = 0, v1 = 0;
  uint8_t n0 = 0, n1 = 0;
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) {
    bool m0 = plan.n_xcap > 0 && plan.xcap_idx[0] == a;
    bool m1 = plan.n_xcap > 1 && plan.xcap_idx[1] == a;
    if (m0 | m1) {
      int64_t v;
      uint8_t nu = 0;
      int k = m0 ? 0 : 1;
      if (!cols[a].found) {
        if (plan.xcap_missing_null[k]) nu = 1;
        v = plan.xcap_missing_val[k];
      } else if (cols[a].null) {
        nu = 1;
        v = 0;
      } else {
        v = cols[a].iv;
      }
      if (m0) { v0 = v; n0 = nu; }
      if (m1) { v1 = v; n1 = nu; }
    }
  }
  *xv0 = v0; *xn0 = n0; *xv1 = v1; *xn1 = n1;
}

/* 128-bit signed accumulate via two u64 atomics (carry trick) */
__device__ static inline void atomic_add_i128(unsigned long long *lo,
                                              unsigned long long *hi, int64_t x) {
  unsigned long long ux = (unsigned long long)x;
  unsigned long long old = atomicAdd(lo, ux);
  unsigned long long carry = (old + ux < old) ? 1ull : 0ull;
  long long hi_add = (long long)carry + (x < 0 ? -1ll : 0ll);
  if (hi_add) atomicAdd(hi, (unsigned long long)hi_add);
}

/* 256-bit signed accumulate: acc = (ext[1] ext[0] hi lo) two's complement;
 * the i128 addend sign-extends into the ext limbs, carries ripple through
 * the returned old values (each limb's add is commutative, carries are
 * explicit later adds, so concurrent updates compose). Wide Decimal sums
 * (decimal.rs:927-942 word_buf range: 38-digit values, 65+-digit sums). */
__device__ static inline void atomic_add_i256(unsigned long long *lo,
                                              unsigned long long *hi,
                                              unsigned long long *ext,
                                              __int128 x) {
  unsigned long long x0 = (unsigned long long)(unsigned __int128)x;
  unsigned long long x1 = (unsigned long long)((unsigned __int128)x >> 64);
  unsigned long long sign = x < 0 ? ~0ull : 0ull;
  unsigned long long o0 = atomicAdd(lo, x0);
  unsigned long long c = (o0 + x0 < o0) ? 1ull : 0ull;
  unsigned long long a1 = x1 + c;
  unsigned long long w1 = (a1 < x1) ? 1ull : 0ull;     /* addend wrapped */
  unsigned long long o1 = atomicAdd(hi, a1);
  c = w1 | ((o1 + a1 < o1) ? 1ull : 0ull);
  unsigned long long a2 = sign + c;
  unsigned long long w2 = (a2 < sign) ? 1ull : 0ull;
  if (a2) {
    unsigned long long o2 = atomicAdd(&ext[0], a2);
    c = w2 | ((o2 + a2 < o2) ? 1ull : 0ull);
  } else {
    c = w2;
  }
  unsigned long long a3 = sign + c;
  if (a3) atomicAdd(&ext[1], a3);
}

/* simple-agg epilogue shared by every mode-1 kernel: per-wave fold of the
 * per-lane partials, then one atomic set per wave per aggregate into the
 * request's accumulators. Must be reached by all 64 lanes of the wave. */
template <int NAGGS>
__device__ static inline void d_simple_epilogue(
    const ScanPlan &plan, SimpleAggAcc *__restrict__ simple_acc,
    const unsigned long long (&l_cnt)[NAGGS],
    const unsigned long long (&l_lo)[NAGGS], const long long (&l_hi)[NAGGS]) {
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) {
    const int32_t kind = plan.aggs[a].kind;
    unsigned long long c = l_cnt[a];
    unsigned long long lo = l_lo[a];
    long long hi = l_hi[a];
    if (d_is_fold(kind)) {
      for (int off = 32; off > 0; off >>= 1) {
        c += (unsigned long long)__shfl_down((long long)c, off, 64);
        unsigned long long plo =
            (unsigned long long)__shfl_down((long long)lo, off, 64);
        if (d_is_xor(kind)) lo ^= plo;
        else if (kind == DAGG_MAX_INT || kind == DAGG_MIN_INT || kind == DAGG_MAX_REAL || kind == DAGG_MIN_REAL)
          lo = lo > plo ? lo : plo;
        else lo |= plo;
      }
      if ((threadIdx.x & 63u) == 0) {
        if (c) atomicAdd(&simple_acc[a].cnt, c);
        if (lo) {
          if (d_is_xor(kind)) atomicXor(&simple_acc[a].sum_lo, lo);
          else if (kind == DAGG_MAX_INT || kind == DAGG_MIN_INT || kind == DAGG_MAX_REAL || kind == DAGG_MIN_REAL)
            atomicMax(&simple_acc[a].sum_lo, lo);
          else atomicOr(&simple_acc[a].sum_lo, lo);
        }
      }
      continue;
    }
    if (kind == DAGG_SUM_REAL) {
      double d = __longlong_as_double((long long)lo);
      for (int off = 32; off > 0; off >>= 1) {
        c += (unsigned long long)__shfl_down((long long)c, off, 64);
        d += __shfl_down(d, off, 64);
      }
      if ((threadIdx.x & 63u) == 0) {
        if (c) atomicAdd(&simple_acc[a].cnt, c);
        if (d != 0.0) atomicAdd((double *)&simple_acc[a].sum_lo, d);
      }
      continue;
    }
    for (int off = 32; off > 0; off >>= 1) {
      c += (unsigned long long)__shfl_down((long long)c, off, 64);
      unsigned long long plo = (unsigned long long)__shfl_down((long long)lo, off, 64);
      long long phi = __shfl_down(hi, off, 64);
      unsigned long long nlo = lo + plo;
      hi += phi + (nlo < lo ? 1 : 0);
      lo = nlo;
    }
    if ((threadIdx.x & 63u) == 0) {
      if (c) atomicAdd(&simple_acc[a].cnt, c);
      if (lo | (unsigned long long)hi) {
        __int128 part = (__int128)(
            ((unsigned __int128)(unsigned long long)hi << 64) | lo);
        if (plan.simple_ext)
          atomic_add_i256(&simple_acc[a].sum_lo, &simple_acc[a].sum_hi,
                          plan.simple_ext + a * 2, part);
        else {
          unsigned long long old = atomicAdd(&simple_acc[a].sum_lo, lo);
          long long carry = (old + lo < old) ? 1 : 0;
          long long hi_add = hi + carry;
          if (hi_add)
            atomicAdd(&simple_acc[a].sum_hi, (unsigned long long)hi_add);
        }
      }
    }
  }
}

/* ---------------- row collector shared by the row-scan kernels ------------
 * What one row yields for a plan: the filter, filter2 and group channels
 * here, and one AggColView per aggregate in an array of the caller's.
 * grp_off is the group cell's offset within the row (GRP_RAW collection
 * only). The array is not a member: the 8-aggregate instances index it
 * dynamically, which keeps it in scratch, and as a member it would take these
 * scalars there with it. */
struct RowVals {
  bool filt_found, filt_null; int64_t filt_v;
  bool f2_found, f2_null; int64_t f2_v;
  bool grp_found, grp_null; int64_t grp_v;
  uint32_t grp_off;
};

__device__ static inline void d_cell_to_col(const CellView &cell,
                                            AggColView *c, bool *parse_ok) {
  c->found = true;
  c->null = cell.is_null;
  c->iv = cell.ival;
  c->has_dec = cell.has_dec;
  c->dsc = cell.dscaled; c->dfr = cell.dfrac;
  c->dwide = cell.dwide; c->dwrem = cell.dwide_rem;
  if (!cell.is_null && !cell.has_int && !cell.has_real && !cell.has_dec &&
      !cell.dwide)
    *parse_ok = false;
}

__device__ static inline void d_cell_to_filter(const CellView &cell,
                                               bool want_real, bool *found,
                                               bool *null, int64_t *v,
                                               bool *parse_ok) {
  *found = true;
  if (cell.is_null) *null = true;
  else if (want_real ? cell.has_real : cell.has_int) *v = cell.ival;
  else *parse_ok = false;
}

/* group cell: an int, or under GRP_RAW with grp_raw set just its offset (the
   caller takes the raw span from there) */
template <bool GRP_RAW>
__device__ static inline void d_cell_to_group(const CellView &cell,
                                              uint32_t cell_off, bool grp_raw,
                                              RowVals &rv,
                                              bool *parse_ok) {
  rv.grp_found = true;
  if (cell.is_null) rv.grp_null = true;
  else if (GRP_RAW && grp_raw) rv.grp_off = cell_off;
  else if (cell.has_int) rv.grp_v = cell.ival;
  else *parse_ok = false;
}

/* Fills rv for the row (vp, vlen) and returns parse_ok: index-key walk in
 * index mode; else one direct next_cell per needed column when the cell
 * directory places them all; else the row-v2 lookup or the row-v1 walk, which
 * stops once every needed column was seen. The group column is looked up only
 * when IS_HASH. dload(slab, col_id) yields the row's directory byte for a
 * column. GRP_RAW (k_scan_extract) and grp_raw: the group cell is wanted as
 * raw bytes, see d_cell_to_group; row-v2 rows then leave the group channel to
 * the caller. Reusing the parsed group value for an aggregate over the group
 * column is the aggregate kernels' (!GRP_RAW) directory branch only. */
template <int NAGGS, bool IS_HASH, bool GRP_RAW, typename DirLoad>
__device__ static inline __attribute__((always_inline)) bool d_row_collect(
    const ScanPlan &plan, const uint8_t *vp, uint32_t vlen, uint64_t my_row,
    DirLoad dload, RowVals &rv, AggColView (&cols)[NAGGS],
    bool grp_raw = false) {
  bool parse_ok = true;
  rv.filt_found = false; rv.filt_null = false; rv.filt_v = 0;
  rv.f2_found = false; rv.f2_null = false; rv.f2_v = 0;
  rv.grp_found = false; rv.grp_null = false; rv.grp_v = 0;
  rv.grp_off = 0;
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) cols[a] = {false, false, false, 0, 0, 0, nullptr, 0};

  if (plan.index_mode) {
    int64_t hval = 0; bool hfound = false;
    parse_ok = d_index_collect<NAGGS, IS_HASH>(plan, vp, vlen, my_row,
                                               &rv.filt_found, &rv.filt_null,
                                               &rv.filt_v, &rv.grp_found,
                                               &rv.grp_null, &rv.grp_v, cols,
                                               &hval, &hfound);
  } else if (!(vlen == 0 || (vlen == 1 && vp[0] == 0))) {
  /* directory fast path: one direct next_cell per needed column instead of a
     sequential walk over every cell */
  bool dir_done = false;
  if (plan.celldir && vp[0] != 128) {
    uint32_t d_f = 0xFFu, d_f2 = 0xFFu, d_g = 0xFFu, d_a[NAGGS];
    if (plan.has_filter) d_f = dload(plan.dirslab_f, plan.filter_col_id);
    if (plan.filter2_on) d_f2 = dload(plan.dirslab_f2, plan.filter2_col_id);
    if (IS_HASH) d_g = dload(plan.dirslab_g, plan.group_col_id);
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      d_a[a] = 0xFFu;
      if (plan.aggs[a].kind != DAGG_COUNT_ROWS)
        d_a[a] = dload(plan.dirslab_a[a], plan.aggs[a].col_id);
    }
    bool seq = (d_f == 0xFEu) | (d_f2 == 0xFEu) | (d_g == 0xFEu);
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) seq |= (d_a[a] == 0xFEu);
    if (!seq) {
      dir_done = true;
      int64_t cid; uint32_t coff; CellView cell; uint32_t pos;
      if (plan.has_filter && d_f != 0xFFu) {
        pos = d_f;
        if (next_cell(vp, vlen, &pos, &cid, &coff, &cell) &&
            cid == plan.filter_col_id)
          d_cell_to_filter(cell, plan.filter_is_real, &rv.filt_found,
                           &rv.filt_null, &rv.filt_v, &parse_ok);
        else parse_ok = false;
      }
      if (plan.filter2_on && d_f2 != 0xFFu) {
        pos = d_f2;
        if (next_cell(vp, vlen, &pos, &cid, &coff, &cell) &&
            cid == plan.filter2_col_id)
          d_cell_to_filter(cell, plan.filter2_is_real, &rv.f2_found,
                           &rv.f2_null, &rv.f2_v, &parse_ok);
        else parse_ok = false;
      }
      if (IS_HASH && d_g != 0xFFu) {
        pos = d_g;
        if (next_cell(vp, vlen, &pos, &cid, &coff, &cell) &&
            cid == plan.group_col_id)
          d_cell_to_group<GRP_RAW>(cell, coff, grp_raw, rv, &parse_ok);
        else parse_ok = false;
      }
      #pragma unroll
      for (int a = 0; a < NAGGS; a++) {
        if (plan.aggs[a].kind == DAGG_COUNT_ROWS || d_a[a] == 0xFFu)
          continue;
        if (IS_HASH && !GRP_RAW && rv.grp_found && !rv.grp_null && parse_ok &&
            plan.aggs[a].col_id == plan.group_col_id &&
            plan.aggs[a].kind != DAGG_SUM_DEC &&
            plan.aggs[a].kind != DAGG_SUM_REAL) {
          /* agg over the GROUP column: reuse the parsed int value
             (avg/sum BY the same column parses the cell once) */
          cols[a].found = true;
          cols[a].null = false;
          cols[a].iv = rv.grp_v;
          continue;
        }
        if (IS_HASH && !GRP_RAW && rv.grp_found && rv.grp_null && parse_ok &&
            plan.aggs[a].col_id == plan.group_col_id) {
          cols[a].found = true;
          cols[a].null = true;
          continue;
        }
        pos = d_a[a];
        if (next_cell(vp, vlen, &pos, &cid, &coff, &cell) &&
            cid == plan.aggs[a].col_id)
          d_cell_to_col(cell, &cols[a], &parse_ok);
        else parse_ok = false;
      }
    }
  }
  if (dir_done) {
  } else if (vp[0] == 128) {   /* row v2 */
    parse_ok = d_v2_collect<NAGGS, IS_HASH>(
        plan, vp, vlen, &rv.filt_found, &rv.filt_null, &rv.filt_v,
        &rv.grp_found, &rv.grp_null, &rv.grp_v, cols, !(GRP_RAW && grp_raw),
        &rv.f2_found, &rv.f2_null, &rv.f2_v);
  } else {
  int needed = (plan.has_filter ? 1 : 0) + (plan.filter2_on ? 1 : 0) + (IS_HASH ? 1 : 0);
  #pragma unroll
  for (int a = 0; a < NAGGS; a++)
    if (plan.aggs[a].kind != DAGG_COUNT_ROWS) needed++;
  int found = 0;
  uint32_t pos = 0;
  while (pos < vlen) {
    int64_t cell_id;
    uint32_t cell_off;
    CellView cell;
    if (!next_cell(vp, vlen, &pos, &cell_id, &cell_off, &cell)) {
      parse_ok = false;
      break;
    }
    if (plan.has_filter && !rv.filt_found && cell_id == plan.filter_col_id) {
      d_cell_to_filter(cell, plan.filter_is_real, &rv.filt_found,
                       &rv.filt_null, &rv.filt_v, &parse_ok);
      found++;
    }
    if (plan.filter2_on && !rv.f2_found && cell_id == plan.filter2_col_id) {
      d_cell_to_filter(cell, plan.filter2_is_real, &rv.f2_found, &rv.f2_null,
                       &rv.f2_v, &parse_ok);
      found++;
    }
    if (IS_HASH && !rv.grp_found && cell_id == plan.group_col_id) {
      d_cell_to_group<GRP_RAW>(cell, cell_off, grp_raw, rv, &parse_ok);
      found++;
    }
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      if (plan.aggs[a].kind == DAGG_COUNT_ROWS || cols[a].found) continue;
      if (cell_id == plan.aggs[a].col_id) {
        d_cell_to_col(cell, &cols[a], &parse_ok);
        found++;
      }
    }
    if (found >= needed) break;
  }
  }  /* v1 walk */
  }  /* non-empty row */
  return parse_ok;
}

/* ---------------- accumulate step shared by the aggregate kernels ---------
 * These are the only implementation of group-slot selection, the
 * per-aggregate update and the LDS-table init and flush: k_scan_agg,
 * k_scan_agg_pipe and k_plane_hash all call them, so a group lands in the
 * same slot with the same accumulator bits whichever kernel saw the row.
 * Stride rule: every accumulator array (ht.accs, ht.ext, ht.reserved,
 * ht.rsvd_ext and the LDS table) is laid out with the plan's n_aggs, never
 * with the NAGGS a kernel instance unrolls to; na = min(n_aggs, NAGGS) and
 * per-aggregate loops skip a >= na. */

/* what the wide-decimal pre-pass and the rescale need to know about one
   sum(decimal) input */
struct DecIn { bool live /* found, not NULL */, wide, has_dec; int64_t sc; int32_t frac; };

/* conservative wide-decimal pre-pass: a row that may need a 256-bit add must
   take a GLOBAL slot (the LDS table is 128-bit). dec_of(a) -> DecIn. */
template <int NAGGS, typename DecOf>
__device__ static inline __attribute__((always_inline)) bool d_row_wide(
    const ScanPlan &plan, DecOf dec_of) {
  bool row_wide = false;
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) {
    if (plan.aggs[a].kind != DAGG_SUM_DEC) continue;
    const DecIn di = dec_of(a);
    if (!di.live) continue;
    if (di.wide) { row_wide = true; continue; }
    if (!di.has_dec) continue;
    int d = plan.aggs[a].target_frac - di.frac;
    if (d > 18) { row_wide = true; continue; }
    if (d > 0) {
      int64_t lim = (int64_t)(0x7FFFFFFFFFFFFFFFll);
      for (int t = 0; t < d; t++) lim /= 10;
      if (di.sc > lim || di.sc < -lim) row_wide = true;
    }
  }
  return row_wide;
}

/* sum(decimal): scale sv (frac digits) to target_frac, 0..38 digits. A value
   that fits an i64 comes back in *v, else in *vw with *dec_wide (the 256-bit
   path). False = frac past the target, or a scaled value past 38 digits. */
__device__ static inline bool d_dec_rescale(__int128 sv, int32_t frac,
                                            int32_t target_frac, int64_t *v,
                                            __int128 *vw, bool *dec_wide) {
  int d = target_frac - frac;
  if (d < 0 || d > 38) return false;
  const __int128 LIM =
      (__int128)(((unsigned __int128)~(unsigned __int128)0) >> 1) / 10;
  for (int t = 0; t < d; t++) {
    if (sv > LIM || sv < -LIM) return false;
    sv *= 10;
  }
  if (sv >= (__int128)INT64_MIN && sv <= (__int128)INT64_MAX) {
    *v = (int64_t)sv;
  } else {
    *vw = sv;
    *dec_wide = true;
  }
  return true;
}

/* one aggregate's value from its collected column: false = no contribution
   (capture-only channel, NULL or absent cell, or a decimal error, which sets
   *err) */
__device__ static inline bool d_agg_value(const DevAggSpec &sp,
                                          const AggColView &c, int64_t *v,
                                          __int128 *vw, bool *dec_wide,
                                          bool *err) {
  if (sp.kind == DAGG_XCAP) return false;          /* capture-only channel */
  if (sp.kind == DAGG_COUNT_ROWS) return true;
  if (!c.found || c.null) return false;
  if (sp.kind == DAGG_COUNT_COL) return true;
  if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_REAL ||
      d_is_fold(sp.kind)) {
    *v = c.iv;
    return true;
  }
  /* SUM_DEC: values to 38 digits via the i128 parse; a scaled value past
     i64 goes to the 256-bit path */
  __int128 sv = 0;
  int32_t fr = 0;
  bool okd = true;
  if (c.has_dec) {
    sv = c.dsc;
    fr = c.dfr;
  } else if (c.dwide) {
    if (!d_decimal_scaled128(c.dwide, c.dwrem, &sv, &fr)) okd = false;
  } else {
    okd = false;
  }
  if (!okd || !d_dec_rescale(sv, fr, sp.target_frac, v, vw, dec_wide)) {
    *err = true;                                   /* loud */
    return false;
  }
  return true;
}

/* PLANE_KINDS = the caller's plans hold only what hash_plane_plan_ok admits:
   count, sum(int), sum(decimal), max(int), min(int). k_plane_hash passes
   true, and the chain of kind tests in its row loop stays as short as those
   kinds need; each test of a by-value plan field costs a spilled-SGPR
   reload there. The arithmetic per kind is the same either way. */
template <bool PLANE_KINDS>
__device__ static inline bool d_fold_kind(int32_t kind) {
  return PLANE_KINDS ? (kind == DAGG_MAX_INT || kind == DAGG_MIN_INT)
                     : d_is_fold(kind);
}

/* fold kinds on an accumulator word: b = the d_fold_xform'd value */
template <bool PLANE_KINDS>
__device__ static inline void d_fold_atomic(int32_t kind,
                                            unsigned long long *w,
                                            unsigned long long b) {
  if (PLANE_KINDS) atomicMax(w, b);
  else if (d_is_xor(kind)) atomicXor(w, b);
  else if (kind == DAGG_MAX_INT || kind == DAGG_MIN_INT ||
           kind == DAGG_MAX_REAL || kind == DAGG_MIN_REAL)
    atomicMax(w, b);
  else atomicOr(w, b);
}

struct HashSlot { SimpleAggAcc *acc; unsigned long long *ext; };

__device__ static inline uint64_t d_group_hash(int64_t key) {
  uint64_t h = (uint64_t)key * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

/* find-or-claim key's slot in the global open-addressed table; a full table
   raises ht.error[0] and returns a null acc (the host grows and retries) */
__device__ static inline HashSlot d_hash_global_slot(const HashAggTable &ht,
                                                     uint32_t table_size,
                                                     uint32_t na,
                                                     int64_t key) {
  const unsigned long long EMPTY = 0x8000000000000000ull;
  HashSlot hs{nullptr, nullptr};
  uint32_t mask = table_size - 1u;
  uint32_t slot = (uint32_t)(d_group_hash(key) & mask);
  for (uint32_t probe = 0; ; probe++) {
    if (probe > mask) { atomicOr(ht.error, 1u); break; }
    unsigned long long curk =
        atomicCAS((unsigned long long *)&ht.keys[slot], EMPTY,
                  (unsigned long long)key);
    if (curk == EMPTY) atomicAdd(ht.n_groups, 1ull);
    if (curk == EMPTY || curk == (unsigned long long)key) {
      hs.acc = ht.accs + (uint64_t)slot * na;
      if (ht.ext) hs.ext = ht.ext + (uint64_t)slot * na * 2;
      break;
    }
    slot = (slot + 1) & mask;
  }
  return hs;
}

/* one kept row's accumulator block: NULL/absent keys -> reserved[1],
   INT64_MIN (the EMPTY sentinel) -> reserved[0], everything else the block's
   LDS pre-aggregation table first (128-bit accumulators, so never for a row
   that may need a 256-bit add) and the global table when that is full */
__device__ static inline HashSlot d_hash_row_slot(
    const HashAggTable &ht, uint32_t table_size, uint32_t na, bool grp_found,
    bool grp_null, int64_t grp_v, bool row_wide, long long *lkeys,
    SimpleAggAcc *laccs, uint32_t lslots) {
  HashSlot hs{nullptr, nullptr};
  if (!grp_found || grp_null) {
    atomicAdd(&ht.rsvd_seen[1], 1ull);
    hs.acc = ht.reserved + 1 * na;
    if (ht.rsvd_ext) hs.ext = ht.rsvd_ext + 1 * na * 2;
    return hs;
  }
  if (grp_v == (long long)0x8000000000000000ll) {
    atomicAdd(&ht.rsvd_seen[0], 1ull);
    hs.acc = ht.reserved;
    if (ht.rsvd_ext) hs.ext = ht.rsvd_ext;
    return hs;
  }
  if (lslots && !row_wide) {
    const unsigned long long EMPTY = 0x8000000000000000ull;
    uint32_t lmask = lslots - 1u;
    uint32_t slot = (uint32_t)(d_group_hash(grp_v) & lmask);
    for (uint32_t probe = 0; probe <= lmask / 2; probe++) {
      unsigned long long curk =
          atomicCAS((unsigned long long *)&lkeys[slot], EMPTY,
                    (unsigned long long)grp_v);
      if (curk == EMPTY || curk == (unsigned long long)grp_v) {
        hs.acc = laccs + (uint64_t)slot * na;
        return hs;
      }
      slot = (slot + 1) & lmask;
    }
  }
  return d_hash_global_slot(ht, table_size, na, grp_v);
}

/* one aggregate's contribution to its accumulator (LDS or global; ext = the
   two high limbs when the accumulator is 256-bit). A 256-bit accumulator
   must see every add as i256: a narrow negative i128 add would not borrow
   from the ext limbs. False = a wide value met a 128-bit accumulator. */
template <bool PLANE_KINDS>
__device__ static inline bool d_hash_update(const DevAggSpec &sp,
                                            SimpleAggAcc *acc,
                                            unsigned long long *ext,
                                            int64_t v, __int128 vw,
                                            bool dec_wide) {
  atomicAdd(&acc->cnt, 1ull);
  if (!PLANE_KINDS && sp.kind == DAGG_SUM_REAL) {
    atomicAdd((double *)&acc->sum_lo, __longlong_as_double(v));
  } else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_DEC) {
    if (ext)
      atomic_add_i256(&acc->sum_lo, &acc->sum_hi, ext,
                      dec_wide ? vw : (__int128)v);
    else if (dec_wide)
      return false;
    else
      atomic_add_i128(&acc->sum_lo, &acc->sum_hi, v);
  } else if (d_fold_kind<PLANE_KINDS>(sp.kind)) {
    d_fold_atomic<PLANE_KINDS>(sp.kind, &acc->sum_lo,
                               d_fold_xform(sp.kind, v, sp.col_unsigned));
  }
  return true;
}

/* prologue: empty the block's LDS pre-aggregation table (lslots keys, then
   lslots * n_aggs accumulators); the caller barriers */
template <int NAGGS>
__device__ static inline void d_hash_lds_init(const ScanPlan &plan,
                                              long long *lkeys,
                                              SimpleAggAcc *laccs,
                                              uint32_t lslots) {
  const uint32_t na = min((uint32_t)plan.n_aggs, (uint32_t)NAGGS);
  for (uint32_t s = threadIdx.x; s < lslots; s += blockDim.x) {
    lkeys[s] = (long long)0x8000000000000000ll;
    #pragma unroll
    for (int a = 0; a < NAGGS; a++)
      if ((uint32_t)a < na) laccs[s * na + a] = SimpleAggAcc{0, 0, 0};
  }
}

/* epilogue: merge the block's LDS pre-aggregation table into the global one */
template <int NAGGS, bool PLANE_KINDS>
__device__ static inline void d_hash_lds_flush(const ScanPlan &plan,
                                               const HashAggTable &ht,
                                               const long long *lkeys,
                                               const SimpleAggAcc *laccs,
                                               uint32_t lslots) {
  const uint32_t na = min((uint32_t)plan.n_aggs, (uint32_t)NAGGS);
  for (uint32_t s = threadIdx.x; s < lslots; s += blockDim.x) {
    long long key = lkeys[s];
    if (key == (long long)0x8000000000000000ll) continue;
    HashSlot gs = d_hash_global_slot(ht, plan.table_size, na, key);
    if (!gs.acc) continue;
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) {
      if ((uint32_t)a >= na) continue;
      const SimpleAggAcc la = laccs[s * na + a];
      const int32_t kind = plan.aggs[a].kind;
      if (la.cnt) atomicAdd(&gs.acc[a].cnt, la.cnt);
      if (d_fold_kind<PLANE_KINDS>(kind)) {
        if (la.sum_lo)
          d_fold_atomic<PLANE_KINDS>(kind, &gs.acc[a].sum_lo, la.sum_lo);
        continue;
      }
      if (la.sum_lo | la.sum_hi) {
        if (gs.ext) {
          atomic_add_i256(&gs.acc[a].sum_lo, &gs.acc[a].sum_hi,
                          gs.ext + a * 2,
                          (__int128)(((unsigned __int128)la.sum_hi << 64) |
                                     la.sum_lo));
        } else {
          unsigned long long old = atomicAdd(&gs.acc[a].sum_lo, la.sum_lo);
          long long carry = (old + la.sum_lo < old) ? 1 : 0;
          long long hi_add = (long long)la.sum_hi + carry;
          if (hi_add) atomicAdd(&gs.acc[a].sum_hi, (unsigned long long)hi_add);
        }
      }
    }
  }
}

/* simple (ungrouped) aggregation: one contribution into the lane's partials,
   folded by d_simple_epilogue. A wide decimal goes straight to the 256-bit
   global accumulator; the per-lane i128 partial keeps only i64-fitting
   values. False = a wide value and no ext buffers. */
__device__ static inline bool d_simple_update(
    const ScanPlan &plan, const DevAggSpec &sp, int a,
    SimpleAggAcc *__restrict__ simple_acc, int64_t v, __int128 vw,
    bool dec_wide, unsigned long long *l_cnt, unsigned long long *l_lo,
    long long *l_hi) {
  (*l_cnt)++;
  if (sp.kind == DAGG_SUM_REAL) {
    *l_lo = (unsigned long long)__double_as_longlong(
        __longlong_as_double((long long)*l_lo) + __longlong_as_double(v));
  } else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_DEC) {
    if (dec_wide) {
      if (!plan.simple_ext) return false;
      atomic_add_i256(&simple_acc[a].sum_lo, &simple_acc[a].sum_hi,
                      plan.simple_ext + a * 2, vw);
    } else {
      unsigned long long old = *l_lo;
      unsigned long long nv = old + (unsigned long long)v;
      *l_hi += (nv < old ? 1 : 0) + (v < 0 ? -1 : 0);
      *l_lo = nv;
    }
  } else if (d_is_fold(sp.kind)) {
    unsigned long long b = d_fold_xform(sp.kind, v, sp.col_unsigned);
    if (d_is_xor(sp.kind)) *l_lo ^= b;
    else if (sp.kind == DAGG_MAX_INT || sp.kind == DAGG_MIN_INT ||
             sp.kind == DAGG_MAX_REAL || sp.kind == DAGG_MIN_REAL)
      *l_lo = *l_lo > b ? *l_lo : b;
    else *l_lo |= b;
  }
  return true;
}

/* One collected row through the keep decision and into the accumulators: the
 * hash table (IS_HASH) or the lane's simple partials. Returns true when the
 * row raised the request's parse error (bad row, keep error, decimal error,
 * wide value without ext buffers). */
template <int NAGGS, bool IS_HASH>
__device__ static inline __attribute__((always_inline)) bool d_row_accumulate(
    const ScanPlan &plan, bool parse_ok, const RowVals &rv,
    const AggColView (&cols)[NAGGS],
    const HashAggTable &ht, long long *lkeys, SimpleAggAcc *laccs,
    uint32_t lslots, SimpleAggAcc *__restrict__ simple_acc,
    unsigned long long (&l_cnt)[NAGGS], unsigned long long (&l_lo)[NAGGS],
    long long (&l_hi)[NAGGS]) {
  int64_t xv0_ = 0, xv1_ = 0;
  uint8_t xn0_ = 0, xn1_ = 0;
  if (plan.n_xcap)
    d_xcap_extract(plan, cols, &xv0_, &xn0_, &xv1_, &xn1_);
  bool err = false;
  if (!parse_ok) {
    err = true;
  } else if (d_keep2(plan, rv.filt_found, rv.filt_null, rv.filt_v,
                     rv.f2_found, rv.f2_null, rv.f2_v, &err, xv0_, xn0_, xv1_,
                     xn1_)) {               /* else dropped, or a keep error */
  const uint32_t na = min((uint32_t)plan.n_aggs, (uint32_t)NAGGS);
  HashSlot hs{nullptr, nullptr};
  if (IS_HASH) {
    const bool row_wide = d_row_wide<NAGGS>(plan, [&](int a) {
      const AggColView &c = cols[a];
      return DecIn{c.found && !c.null, c.dwide != nullptr, c.has_dec, c.dsc,
                   c.dfr};
    });
    hs = d_hash_row_slot(ht, plan.table_size, na, rv.grp_found, rv.grp_null,
                         rv.grp_v, row_wide, lkeys, laccs, lslots);
  }
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) {
    if (IS_HASH && (uint32_t)a >= na) continue;
    const DevAggSpec &sp = plan.aggs[a];
    bool dec_wide = false;       /* value does not fit a scaled i64 */
    __int128 vw = 0;
    int64_t v = 0;
    if (!d_agg_value(sp, cols[a], &v, &vw, &dec_wide, &err)) continue;
    if (IS_HASH) {
      if (hs.acc &&
          !d_hash_update<false>(sp, hs.acc + a,
                                hs.ext ? hs.ext + a * 2 : nullptr, v, vw,
                                dec_wide))
        err = true;                      /* no ext buffers: loud */
    } else if (!d_simple_update(plan, sp, a, simple_acc, v, vw, dec_wide,
                                &l_cnt[a], &l_lo[a], &l_hi[a])) {
      err = true;
    }
  }
  }
  return err;
}

/* ---------------- fused scan + filter + aggregate ----------------
 * NAGGS is a compile-time bound so all per-row/per-lane state stays in
 * registers. IS_HASH selects grouped aggregation. Single LDS buffer: the
 * block stages one tile with stage_tile, barriers, and every lane parses its
 * rows from LDS (d_row_collect, d_row_accumulate) before the next tile is
 * staged. */
template <int NAGGS, bool IS_HASH>
__global__ void __launch_bounds__(THREADS, 2)
k_scan_agg(ScanPlan plan,
           const uint8_t *__restrict__ vals, const uint64_t *__restrict__ val_offs,
           uint64_t n_rows,
           SimpleAggAcc *__restrict__ simple_acc,
           HashAggTable ht) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

  const uint32_t rpt = plan.rows_per_tile;
  const uint64_t n_tiles = (n_rows + rpt - 1) / rpt;

  unsigned long long l_cnt[NAGGS];
  unsigned long long l_lo[NAGGS];
  long long l_hi[NAGGS];
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) { l_cnt[a] = 0; l_lo[a] = 0; l_hi[a] = 0; }

  bool any_parse_err = false;

  /* per-block LDS pre-aggregation table (hash mode): keys + accumulators
     after the tile region. Cuts global atomic contention ~rows/slots-fold
     for low-cardinality GROUP BY. */
  long long *lkeys = nullptr;
  SimpleAggAcc *laccs = nullptr;
  const uint32_t LSLOTS = IS_HASH ? plan.lds_agg_slots : 0;
  if (IS_HASH && LSLOTS) {
    lkeys = (long long *)(lds + plan.lds_agg_off);
    laccs = (SimpleAggAcc *)(lkeys + LSLOTS);
    d_hash_lds_init<NAGGS>(plan, lkeys, laccs, LSLOTS);
    __syncthreads();
  }

  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    uint64_t gbase = val_offs[row0];
    uint32_t tlen = (uint32_t)(val_offs[row1] - gbase);
    __syncthreads();                    /* previous parse done: LDS free */
    uint32_t shift = stage_tile(vals, gbase, tlen, lds);

    for (uint64_t my_row = row0 + threadIdx.x; my_row < row1; my_row += blockDim.x) {
      const uint8_t *vp = lds + shift + (uint32_t)(val_offs[my_row] - gbase);
      uint32_t vlen = (uint32_t)(val_offs[my_row + 1] - val_offs[my_row]);
      RowVals rv;
      AggColView cols[NAGGS];
      const uint8_t *db = plan.celldir;
      const uint64_t dn = plan.celldir_n;
      bool parse_ok = d_row_collect<NAGGS, IS_HASH, false>(
          plan, vp, vlen, my_row,
          [&](int32_t, int64_t cid) -> uint32_t {
            return (uint32_t)db[(uint64_t)(cid - 1) * dn + my_row];
          },
          rv, cols);
      any_parse_err |= d_row_accumulate<NAGGS, IS_HASH>(
          plan, parse_ok, rv, cols, ht, lkeys, laccs, LSLOTS, simple_acc, l_cnt,
          l_lo, l_hi);
    }
  }

  /* flush the block's LDS pre-agg table into the global table */
  if (IS_HASH && LSLOTS) {
    __syncthreads();
    d_hash_lds_flush<NAGGS, false>(plan, ht, lkeys, laccs, LSLOTS);
  }

  if (!IS_HASH) d_simple_epilogue<NAGGS>(plan, simple_acc, l_cnt, l_lo, l_hi);
  if (any_parse_err) {
    if (IS_HASH) atomicOr(ht.error + 1, 1u);
    else atomicOr((unsigned int *)&simple_acc[COPR_MAX_AGGS].cnt, 1u);
  }
}

/* ---------------- glds-pipelined scan + filter + aggregate ----------------
 * Two LDS buffers; tile t+1's bytes (offsets slab + values slab) stream
 * HBM->LDS via __builtin_amdgcn_global_load_lds WHILE lanes parse tile t:
 * issue(next) -> parse(cur) -> s_waitcnt vmcnt(0) -> barrier -> swap. The
 * parse touches no vector global loads (per-row offsets come from the LDS
 * offs slab), so hipcc inserts no early vmcnt(0) that would drain the DMA
 * queue (cdna_hip_programming §5 pipelining-across-barriers / §6 G15). */
template <int NAGGS, bool IS_HASH, bool FASTFC = false>
__global__ void __launch_bounds__(THREADS, 2)
k_scan_agg_pipe(ScanPlan plan,
                const uint8_t *__restrict__ vals,
                const uint64_t *__restrict__ val_offs, uint64_t n_rows,
                SimpleAggAcc *__restrict__ simple_acc, HashAggTable ht) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t rpt = plan.rows_per_tile;
  const uint64_t n_tiles = (n_rows + rpt - 1) / rpt;
  const uint32_t OS = plan.offs_slab;
  const uint32_t DS = plan.dir_slab;          /* dir slice after the values */
  const uint32_t BUFSZ = OS + plan.vals_slab + DS;
  const uint32_t DOFF = OS + plan.vals_slab;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t nwaves = THREADS / 64u;

  unsigned long long l_cnt[NAGGS];
  unsigned long long l_lo[NAGGS];
  long long l_hi[NAGGS];
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) { l_cnt[a] = 0; l_lo[a] = 0; l_hi[a] = 0; }

  bool any_parse_err = false;

  /* per-block LDS pre-aggregation table (hash mode, after the two DMA
     buffers): cuts global atomic contention ~rows/slots-fold for
     low-cardinality GROUP BY (same structure as k_scan_agg's) */
  long long *lkeys = nullptr;
  SimpleAggAcc *laccs = nullptr;
  const uint32_t LSLOTS = IS_HASH ? plan.lds_agg_slots : 0;
  if (IS_HASH && LSLOTS) {
    lkeys = (long long *)(lds + plan.lds_agg_off);
    laccs = (SimpleAggAcc *)(lkeys + LSLOTS);
    d_hash_lds_init<NAGGS>(plan, lkeys, laccs, LSLOTS);
    __syncthreads();
  }

  /* issue the HBM->LDS DMA for a tile whose bounds (gb, ge) are ALREADY in
     registers — no loads between glds issues, so no compiler vmcnt lands in
     the middle of the queue */
  auto issue_tile = [&](uint64_t tile, uint8_t *b, uint64_t gb, uint64_t ge) {
    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    /* offsets slab: val_offs[row0 .. row1] raw (1 KiB chunks, whole-chunk
       over-read stays inside the +2 KiB region slack) */
    const uint8_t *osrc = (const uint8_t *)(val_offs + row0);
    uint32_t obytes = (uint32_t)((row1 - row0 + 1) * 8);
    uint32_t oc = (obytes + 1023u) >> 10;
    for (uint32_t c = wave; c < oc; c += nwaves) {
      uint32_t off = (c << 10) + lane * 16u;
      __builtin_amdgcn_global_load_lds((const uint32_t *)(osrc + off),
                                       (uint32_t *)(b + off), 16, 0, 0);
    }
    /* values slab, 16-aligned from the tile's aligned base */
    uint64_t abase = gb & ~15ull;
    uint32_t tbytes = (uint32_t)(ge - abase);
    uint32_t vc = (tbytes + 1023u) >> 10;
    const uint8_t *vsrc = vals + abase;
    uint8_t *bv = b + OS;
    for (uint32_t c = wave; c < vc; c += nwaves) {
      uint32_t off = (c << 10) + lane * 16u;
      __builtin_amdgcn_global_load_lds((const uint32_t *)(vsrc + off),
                                       (uint32_t *)(bv + off), 16, 0, 0);
    }
    /* tile slices of the needed directory planes: rpt <= 1024 bytes each =
       one 1 KiB chunk per slab (row0 is rpt-aligned, planes have tail
       slack). Slab k staged by wave (nwaves-1-k)%nwaves so slab 0 keeps
       its historical wave. */
    if (DS) {
      if (plan.n_dir_slabs > 0) {
        for (int32_t k2 = 0; k2 < plan.n_dir_slabs; k2++) {
          if (wave != (nwaves - 1u - ((uint32_t)k2 % nwaves))) continue;
          const uint8_t *dsrc = plan.dir_planes_staged[k2] + row0;
          __builtin_amdgcn_global_load_lds(
              (const uint32_t *)(dsrc + lane * 16u),
              (uint32_t *)(b + DOFF + (uint32_t)k2 * 1024u + lane * 16u),
              16, 0, 0);
        }
      } else if (wave == nwaves - 1) {
        const uint8_t *dsrc = plan.dir_plane + row0;
        __builtin_amdgcn_global_load_lds((const uint32_t *)(dsrc + lane * 16u),
                                         (uint32_t *)(b + DOFF + lane * 16u),
                                         16, 0, 0);
      }
    }
  };
  auto bounds_of = [&](uint64_t tile, uint64_t *gb, uint64_t *ge) {
    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    *gb = val_offs[row0];
    *ge = val_offs[row1];
  };

  uint64_t tile = blockIdx.x;
  uint32_t bsel = 0;
  uint64_t nb_gb = 0, nb_ge = 0;        /* bounds of tile+gridDim, in flight */
  if (tile < n_tiles) {
    uint64_t gb, ge;
    bounds_of(tile, &gb, &ge);
    issue_tile(tile, lds, gb, ge);
    bounds_of(min(tile + gridDim.x, n_tiles - 1), &nb_gb, &nb_ge);
  }

  for (; tile < n_tiles; tile += gridDim.x) {
    /* ONE drain per tile: current tile's DMA (issued last iteration, landed
       during the previous parse) + the prefetched next-tile bounds */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint8_t *b = lds + bsel * BUFSZ;
    uint8_t *bn = lds + (bsel ^ 1) * BUFSZ;
    uint64_t next = tile + gridDim.x;
    if (next < n_tiles) issue_tile(next, bn, nb_gb, nb_ge);
    bounds_of(min(next + gridDim.x, n_tiles - 1), &nb_gb, &nb_ge);

    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    const uint64_t *loffs = (const uint64_t *)b;
    uint64_t gb = loffs[0];
    uint32_t shift = (uint32_t)(gb & 15ull);
    const uint8_t *bv = b + OS;

    if (FASTFC) {
      /* specialized: one int filter column + count(*) — the cfg2 shape.
         Streaming 16-byte register window over the row: ~1 ds_read_b64 pair
         per two cells, no value extraction for non-target cells. */
      const int64_t FCID = plan.filter_col_id;
      const uint8_t *DIRP = plan.dir_plane;
      const uint8_t *b_dir = b + DOFF;
      unsigned long long cnt = 0;
      for (uint64_t my_row = row0 + threadIdx.x; my_row < row1; my_row += blockDim.x) {
        uint32_t dir8 = DS ? (uint32_t)b_dir[my_row - row0]
                           : (DIRP ? (uint32_t)DIRP[my_row] : 0xFEu);
        uint32_t r = (uint32_t)(my_row - row0);
        uint64_t o0 = loffs[r], o1 = loffs[r + 1];
        const uint8_t *vp = bv + shift + (uint32_t)(o0 - gb);
        uint32_t vlen = (uint32_t)(o1 - o0);
        bool found = false, fnull = false, ok = true;
        int64_t fv = 0;
        if (dir8 == 0xFFu) {
          /* directory: filter column absent in this row -> default fill */
        } else if (!(vlen == 0 || (vlen == 1 && vp[0] == 0))) {
          if (vp[0] == 128) {        /* row v2: direct column lookup */
            V2Row r;
            if (!d_v2_parse(vp, vlen, &r)) ok = false;
            else {
              uint32_t s, e;
              int st = d_v2_find(r, FCID, &s, &e);
              if (st >= 0) {
                found = true;
                if (st == 0) fnull = true;
                else if (!d_v2_int(r.vals + s, e - s,
                                   plan.filter_col_unsigned, &fv))
                  ok = false;
              }
            }
          } else {
          uintptr_t base = (uintptr_t)vp;
          uintptr_t wabs = ~(uintptr_t)0;   /* window invalid */
          uint64_t wlo = 0, whi = 0;
          /* directory hit: jump straight to the filter column's cell (the
             while body then matches on its first iteration) */
          uint32_t pos = dir8 < 0xFEu ? dir8 : 0u;
          while (pos < vlen) {
            uintptr_t ua = base + pos;
            if (ua - wabs > 8) {            /* reload 16B window */
              wabs = ua & ~(uintptr_t)7;
              const uint64_t *q = (const uint64_t *)wabs;
              wlo = q[0];
              whi = q[1];
            }
            uint32_t sh = (uint32_t)(ua - wabs) * 8u;
            uint64_t x;
            if (sh == 0) x = wlo;
            else if (sh == 64) x = whi;
            else x = (wlo >> sh) | (whi << (64 - sh));
            if ((x & 0xFF) != 8) { ok = false; break; }
            uint32_t b1 = (uint32_t)(x >> 8) & 0xFF;
            uint32_t dflag = (uint32_t)(x >> 16) & 0xFF;
            if (b1 < 0x80 && (dflag == 8 || dflag == 9)) {
              uint64_t m = x >> 24;
              uint64_t stops = ~m & 0x8080808080ull;
              if (stops) {
                uint32_t half = b1 >> 1;
                int64_t cid = (b1 & 1) ? (int64_t)(~(uint64_t)half) : (int64_t)half;
                uint32_t n = ((uint32_t)__ffsll((long long)stops)) >> 3;
                if (cid == FCID) {
                  uint64_t vm = m & ((n == 5) ? 0xFFFFFFFFFFull
                                              : ((1ull << (8 * n)) - 1));
                  uint64_t uv = (vm & 0x7f) | ((vm >> 8) & 0x7f) << 7 |
                                ((vm >> 16) & 0x7f) << 14 |
                                ((vm >> 24) & 0x7f) << 21 |
                                ((vm >> 32) & 0x7f) << 28;
                  if (dflag == 8) {
                    uint64_t h2 = uv >> 1;
                    fv = (uv & 1) ? (int64_t)~h2 : (int64_t)h2;
                  } else {
                    fv = (int64_t)uv;
                  }
                  found = true;
                  break;
                }
                pos += 3 + n;
                continue;
              }
            }
            /* uncommon cell: generic parser for this cell */
            {
              int64_t cid;
              uint32_t cell_off;
              CellView cell;
              if (!next_cell(vp, vlen, &pos, &cid, &cell_off, &cell)) { ok = false; break; }
              if (cid == FCID) {
                if (cell.is_null) fnull = true;
                else if (plan.filter_is_real ? cell.has_real : cell.has_int) fv = cell.ival;
                else ok = false;
                found = true;
                break;
              }
            }
          }
          }  /* v1/v2 */
        }
        if (!ok) any_parse_err = true;
        else if (d_filter_keep(plan, found, fnull, fv)) cnt++;
      }
      l_cnt[0] += cnt;
    } else {
    for (uint64_t my_row = row0 + threadIdx.x; my_row < row1; my_row += blockDim.x) {
      uint32_t r = (uint32_t)(my_row - row0);
      uint64_t o0 = loffs[r], o1 = loffs[r + 1];
      const uint8_t *vp = bv + shift + (uint32_t)(o0 - gb);
      uint32_t vlen = (uint32_t)(o1 - o0);
      RowVals rv;
      AggColView cols[NAGGS];
      const uint8_t *db = plan.celldir;
      const uint64_t dn = plan.celldir_n;
      /* dir bytes come from the DMA-staged tile slices when assigned
         (they head the parse dependency chain; a per-row random global
         load here parks the wave ~L2/HBM latency per row) */
      const uint8_t *b_dirs = b + DOFF;
      bool parse_ok = d_row_collect<NAGGS, IS_HASH, false>(
          plan, vp, vlen, my_row,
          [&](int32_t slab, int64_t cid) -> uint32_t {
            return (DS && slab >= 0)
                       ? (uint32_t)b_dirs[(uint32_t)slab * 1024u + r]
                       : (uint32_t)db[(uint64_t)(cid - 1) * dn + my_row];
          },
          rv, cols);
      any_parse_err |= d_row_accumulate<NAGGS, IS_HASH>(
          plan, parse_ok, rv, cols, ht, lkeys, laccs, LSLOTS, simple_acc, l_cnt,
          l_lo, l_hi);
    }
    }  /* FASTFC else */
    bsel ^= 1;
  }

  /* flush the block's LDS pre-agg table into the global table */
  if (IS_HASH && LSLOTS) {
    __syncthreads();
    d_hash_lds_flush<NAGGS, false>(plan, ht, lkeys, laccs, LSLOTS);
  }

  if (!IS_HASH) d_simple_epilogue<NAGGS>(plan, simple_acc, l_cnt, l_lo, l_hi);
  if (any_parse_err) {
    if (IS_HASH) atomicOr(ht.error + 1, 1u);
    else atomicOr((unsigned int *)&simple_acc[COPR_MAX_AGGS].cnt, 1u);
  }
}

/* ---------------- cell-directory ingest ----------------
 * One-time pass at region load: per row, walk the row-v1 cells byte-wise
 * from GLOBAL memory (codec::row walk, components/tidb_query_datum_codec)
 * and record each small-id cell's start offset into 16 column-major byte
 * planes. All per-row state lives in two packed u64s (no local arrays ->
 * no scratch). */
__device__ static inline uint32_t d_dec_bin_size(uint32_t prec, uint32_t frac) {
  const uint32_t dig2b[10] = {0, 1, 1, 2, 2, 3, 3, 4, 4, 4};
  uint32_t intg = prec - frac;
  return (intg / 9) * 4 + dig2b[intg % 9] + (frac / 9) * 4 + dig2b[frac % 9];
}

__global__ void __launch_bounds__(256)
k_build_celldir(const uint8_t *__restrict__ vals,
                const uint64_t *__restrict__ val_offs, uint64_t n_rows,
                uint8_t *__restrict__ dir) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < n_rows; row += stride) {
    uint64_t o0 = val_offs[row], o1 = val_offs[row + 1];
    const uint8_t *vp = vals + o0;
    uint32_t vlen = (uint32_t)(o1 - o0);
    uint64_t plo = ~0ull, phi = ~0ull;       /* 16 x 0xFF (absent) */
    bool bad = false;
    if (vlen == 0 || (vlen == 1 && vp[0] == 0) || vp[0] == 128) {
      bad = true;                            /* empty / v2: generic path */
    } else {
      uint32_t pos = 0;
      while (pos < vlen && !bad) {
        uint32_t cell_start = pos;
        if (pos + 2 > vlen || vp[pos] != 8) { bad = true; break; }
        uint32_t b1 = vp[pos + 1];
        int64_t cid;
        uint32_t p = pos + 2;
        if (b1 < 0x80) {
          uint32_t half = b1 >> 1;
          cid = (b1 & 1) ? (int64_t)(~(uint64_t)half) : (int64_t)half;
        } else {                              /* multi-byte zigzag id */
          uint64_t uv = (uint64_t)(b1 & 0x7F);
          uint32_t sh = 7;
          bool done = false;
          while (p < vlen && sh < 70) {
            uint8_t by = vp[p++];
            uv |= (uint64_t)(by & 0x7F) << sh;
            sh += 7;
            if (!(by & 0x80)) { done = true; break; }
          }
          if (!done) { bad = true; break; }
          uint64_t half = uv >> 1;
          cid = (uv & 1) ? (int64_t)(~half) : (int64_t)half;
        }
        if (p >= vlen) { bad = true; break; }
        uint8_t f = vp[p];                    /* value datum flag */
        uint32_t adv = 0;
        switch (f) {
          case 0: adv = 1; break;             /* NIL */
          case 3: case 4: case 5: case 7:     /* INT/UINT/FLOAT/DURATION */
            adv = 9; break;
          case 8: case 9: {                   /* VAR_INT / VAR_UINT */
            uint32_t q = p + 1, n = 0;
            while (q < vlen && n < 10 && (vp[q] & 0x80)) { q++; n++; }
            if (q >= vlen) { bad = true; }
            adv = q + 1 - p;
            break;
          }
          case 1: {                           /* BYTES (memcomparable) */
            uint32_t q = p + 1;
            for (;;) {
              if (q + 9 > vlen) { bad = true; break; }
              uint8_t m = vp[q + 8];
              q += 9;
              if (m != 0xFF) break;
            }
            adv = q - p;
            break;
          }
          case 2: {                           /* COMPACT_BYTES */
            uint32_t q = p + 1;
            uint64_t uv = 0; uint32_t sh = 0; bool done = false;
            while (q < vlen && sh < 70) {
              uint8_t by = vp[q++];
              uv |= (uint64_t)(by & 0x7F) << sh;
              sh += 7;
              if (!(by & 0x80)) { done = true; break; }
            }
            int64_t n = (uv & 1) ? (int64_t)(~(uv >> 1)) : (int64_t)(uv >> 1);
            if (!done || n < 0) { bad = true; break; }
            adv = (q - p) + (uint32_t)n;
            break;
          }
          case 6: {                           /* DECIMAL: [prec][frac][bin] */
            if (p + 3 > vlen) { bad = true; break; }
            adv = 3 + d_dec_bin_size(vp[p + 1], vp[p + 2]);
            break;
          }
          default: bad = true; break;
        }
        if (bad) break;
        pos = p + adv;
        if (pos > vlen) { bad = true; break; }
        if (cid >= 1 && cid <= 16) {
          uint32_t c = (uint32_t)(cid - 1);
          uint64_t v = (cell_start < 254) ? (uint64_t)cell_start : 0xFEull;
          uint32_t sh = (c & 7) * 8;
          if (c < 8) plo = (plo & ~(0xFFull << sh)) | (v << sh);
          else       phi = (phi & ~(0xFFull << sh)) | (v << sh);
        }
      }
    }
    if (bad) { plo = 0xFEFEFEFEFEFEFEFEull; phi = plo; }
    #pragma unroll
    for (uint32_t c = 0; c < 16; c++) {
      uint64_t w = c < 8 ? plo : phi;
      dir[(uint64_t)c * n_rows + row] = (uint8_t)(w >> ((c & 7) * 8));
    }
  }
}

int dev_celldir_build(DevRegion &rgn, hipStream_t s) {
  if (!rgn.n_kv) return 0;
  hipError_t e = hipMalloc((void **)&rgn.d_celldir, rgn.n_kv * 16 + 2048);
  if (e != hipSuccess) { rgn.d_celldir = nullptr; return 0; /* optional */ }
  uint32_t grid = (uint32_t)min((rgn.n_kv + 255) / 256, (uint64_t)16384);
  hipLaunchKernelGGL(k_build_celldir, dim3(grid), dim3(256), 0, s,
                     rgn.d_vals, rgn.d_val_offs, rgn.n_kv, rgn.d_celldir);
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) { hipFree(rgn.d_celldir); rgn.d_celldir = nullptr; }
  return 0;
}

/* ---------------- decoded column planes ----------------
 * A filter/count request decides each row from ~7 of the ~126 bytes the scan
 * kernels stage. A plane keeps, per (region, column), the decoded i64 value
 * and a state byte for every row, so simple aggregates over int/real columns
 * read 9 bytes per row per column instead of the whole row. */

/* Locate column col_id's cell in one row exactly as the scan kernels do.
 * dir8 is the row's cell-directory byte for the column (0xFE when the region
 * has no directory): a hit inspects the target cell alone, 0xFF is absent,
 * 0xFE walks the row and stops at the column. Reads global memory
 * (next_cell takes generic pointers). */
enum { LOC_ABSENT = 0, LOC_CELL, LOC_ERR, LOC_V2 };
__device__ static inline int d_col_locate(const uint8_t *vp, uint32_t vlen,
                                          uint32_t dir8, int64_t col_id,
                                          CellView *cell) {
  if (vlen == 0 || (vlen == 1 && vp[0] == 0)) return LOC_ABSENT;
  if (vp[0] == 128) return LOC_V2;
  int64_t cid;
  uint32_t coff;
  /* next_cell's word path leaves these untouched */
  cell->has_real = false;
  cell->has_dec = false;
  cell->dwide = nullptr;
  cell->ival = 0;
  if (dir8 == 0xFFu) return LOC_ABSENT;
  if (dir8 < 0xFEu) {
    uint32_t pos = dir8;
    if (next_cell(vp, vlen, &pos, &cid, &coff, cell) && cid == col_id)
      return LOC_CELL;
    return LOC_ERR;
  }
  uint32_t pos = 0;
  while (pos < vlen) {
    if (!next_cell(vp, vlen, &pos, &cid, &coff, cell)) return LOC_ERR;
    if (cid == col_id) return LOC_CELL;
  }
  return LOC_ABSENT;
}

/* One-time pass per (region, column): classify every row's cell and store
 * the decoded value. n_rowparse counts the rows left to query time. */
__global__ void __launch_bounds__(256)
k_build_colplane(const uint8_t *__restrict__ vals,
                 const uint64_t *__restrict__ val_offs, uint64_t n_rows,
                 const uint8_t *__restrict__ dirp, int64_t col_id,
                 int64_t *__restrict__ pval, uint8_t *__restrict__ pst,
                 unsigned long long *__restrict__ n_rowparse /* [2]: +dec */) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long rp = 0, nd = 0;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < n_rows; row += stride) {
    uint64_t o0 = val_offs[row], o1 = val_offs[row + 1];
    uint32_t dir8 = dirp ? (uint32_t)dirp[row] : 0xFEu;
    CellView cell;
    int64_t v = 0;
    uint8_t st;
    switch (d_col_locate(vals + o0, (uint32_t)(o1 - o0), dir8, col_id, &cell)) {
      case LOC_ABSENT: st = PST_ABSENT; break;
      case LOC_ERR:    st = PST_ERR; break;
      case LOC_V2:     st = PST_ROWPARSE; break;
      default:
        if (cell.is_null) st = PST_NULL;
        else if (cell.has_int) { st = PST_INT; v = cell.ival; }
        else if (cell.has_real) { st = PST_REAL; v = cell.ival; }
        else if (cell.has_dec && (uint32_t)cell.dfrac <= 18u) {
          /* has_dec means prec <= 18, so frac fits beside PST_DEC0 */
          st = (uint8_t)(PST_DEC0 + cell.dfrac);
          v = cell.dscaled;
        }
        else st = PST_ROWPARSE;
        break;
    }
    pval[row] = v;
    pst[row] = st;
    rp += st == PST_ROWPARSE ? 1ull : 0ull;
    nd += st >= PST_DEC0 ? 1ull : 0ull;
  }
  for (int off = 32; off > 0; off >>= 1) {
    rp += (unsigned long long)__shfl_down((long long)rp, off, 64);
    nd += (unsigned long long)__shfl_down((long long)nd, off, 64);
  }
  if ((threadIdx.x & 63u) == 0 && rp) atomicAdd(n_rowparse, rp);
  if ((threadIdx.x & 63u) == 0 && nd) atomicAdd(n_rowparse + 1, nd);
}

void dev_colplane_free(DevRegion &rgn) {
  for (int32_t i = 0; i < rgn.n_planes; i++) {
    hipFree(rgn.planes[i].val);
    hipFree(rgn.planes[i].st);
    hipFree(rgn.planes[i].nar);
    rgn.planes[i] = DevRegion::ColPlane{};
  }
  rgn.n_planes = 0;
  rgn.plane_bytes = 0;
}

const DevRegion::ColPlane *dev_colplane_get(DevRegion &rgn, int64_t col_id,
                                            uint64_t budget_bytes,
                                            hipStream_t s, uint64_t *built) {
  for (int32_t i = 0; i < rgn.n_planes; i++)
    if (rgn.planes[i].col_id == col_id)
      return rgn.planes[i].val ? &rgn.planes[i] : nullptr;
  if (!rgn.n_kv || rgn.n_planes == COPR_MAX_PLANES) return nullptr;
  const uint64_t cost = rgn.n_kv * 9;
  if (rgn.plane_bytes + cost > budget_bytes) return nullptr;
  DevRegion::ColPlane p{};
  p.col_id = col_id;
  unsigned long long *d_rp = nullptr;   /* [0] ROWPARSE rows, [1] decimal rows */
  unsigned long long h_rp[2] = {0, 0};
  /* tail slack like the directory's: the plane kernel's 16 B loads round
     the last pair up */
  hipError_t e = hipMalloc((void **)&p.val, rgn.n_kv * 8 + 2048);
  if (e == hipSuccess) e = hipMalloc((void **)&p.st, rgn.n_kv + 2048);
  if (e == hipSuccess) e = hipMalloc((void **)&d_rp, 16);
  if (e == hipSuccess) e = hipMemsetAsync(d_rp, 0, 16, s);
  if (e == hipSuccess) {
    const uint8_t *dirp =
        (rgn.d_celldir && col_id >= 1 && col_id <= 16)
            ? rgn.d_celldir + (uint64_t)(col_id - 1) * rgn.n_kv : nullptr;
    uint32_t grid = (uint32_t)min((rgn.n_kv + 255) / 256, (uint64_t)16384);
    hipLaunchKernelGGL(k_build_colplane, dim3(grid), dim3(256), 0, s,
                       rgn.d_vals, rgn.d_val_offs, rgn.n_kv, dirp, col_id,
                       p.val, p.st, d_rp);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_rp, d_rp, 16, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d_rp);
  if (e != hipSuccess) {             /* optional, like the directory */
    (void)hipGetLastError();
    hipFree(p.val);
    hipFree(p.st);
    return nullptr;
  }
  DevRegion::ColPlane &slot = rgn.planes[rgn.n_planes++];
  if (h_rp[0] * 8 > rgn.n_kv) {
    /* mostly rows that need the row bytes anyway (row-v2 region, wide
       decimal or bytes column): the scan path reads less. Remember the
       verdict. Decimal rows are not counted: k_plane_hash reads them from
       the plane, and the simple consumer declines per request. */
    hipFree(p.val);
    hipFree(p.st);
    slot = DevRegion::ColPlane{};
    slot.col_id = col_id;
    return nullptr;
  }
  p.n_rowparse = h_rp[0];
  p.n_dec = h_rp[1];
  slot = p;
  rgn.plane_bytes += cost;
  if (built) (*built)++;
  return &slot;
}

/* One plane channel for one row -> what the scan kernels' collect step
 * produces for the column: value + CH_* flags. want: 0 int filter, 1 real
 * filter, 2 int-valued aggregate (sum/max/min), 3 count(col). */
enum { CH_FOUND = 1, CH_NULL = 2, CH_ERR = 4 };
struct ChanRes { int64_t v; uint32_t fl; };

/* ROWPARSE rows: resolve the column from the row bytes with the request's
 * signedness / type. Rare, so kept out of line to leave the streaming loop
 * small. */
__device__ __noinline__ static ChanRes d_plane_resolve(
    const uint8_t *dirp, uint64_t row, int64_t col_id, bool uns, int want,
    const uint8_t *vals, const uint64_t *val_offs) {
  ChanRes cr{0, 0};
  uint64_t o0 = val_offs[row], o1 = val_offs[row + 1];
  const uint8_t *vp = vals + o0;
  uint32_t vlen = (uint32_t)(o1 - o0);
  uint32_t dir8 = dirp ? (uint32_t)dirp[row] : 0xFEu;
  CellView cell;
  int loc = d_col_locate(vp, vlen, dir8, col_id, &cell);
  if (loc == LOC_ERR) {
    cr.fl = CH_ERR;
  } else if (loc == LOC_V2) {
    V2Row r;
    uint32_t s, e;
    if (!d_v2_parse(vp, vlen, &r)) { cr.fl = CH_ERR; return cr; }
    int fs = d_v2_find(r, col_id, &s, &e);
    if (fs < 0) return cr;
    cr.fl = CH_FOUND;
    if (fs == 0) { cr.fl |= CH_NULL; return cr; }
    if (want == 1) {
      if (e - s != 8) { cr.fl |= CH_ERR; return cr; }
      uint64_t u = d_be_u64(r.vals + s);
      cr.v = (int64_t)((u & 0x8000000000000000ull)
                           ? (u ^ 0x8000000000000000ull) : ~u);
    } else if (want != 3) {
      if (!d_v2_int(r.vals + s, e - s, uns, &cr.v)) cr.fl |= CH_ERR;
    }
  } else if (loc == LOC_CELL) {
    cr.fl = CH_FOUND;
    if (want <= 1) {
      if (cell.is_null) cr.fl |= CH_NULL;
      else if (want == 1 ? cell.has_real : cell.has_int) cr.v = cell.ival;
      else cr.fl |= CH_ERR;
    } else {
      if (cell.is_null) cr.fl |= CH_NULL;
      cr.v = cell.ival;
      if (!cell.is_null && !cell.has_int && !cell.has_real &&
          !cell.has_dec && !cell.dwide)
        cr.fl |= CH_ERR;
    }
  }
  return cr;
}

__device__ static inline ChanRes d_plane_chan(
    const PlaneRef &pr, uint32_t st, int64_t pv, uint64_t row, int64_t col_id,
    bool uns, int want, const uint8_t *vals, const uint64_t *val_offs) {
  switch (st) {
    case PST_INT:    return ChanRes{pv, want == 1 ? (uint32_t)(CH_FOUND | CH_ERR)
                                                  : (uint32_t)CH_FOUND};
    case PST_REAL:   return ChanRes{pv, want == 0 ? (uint32_t)(CH_FOUND | CH_ERR)
                                                  : (uint32_t)CH_FOUND};
    case PST_NULL:   return ChanRes{0, CH_FOUND | CH_NULL};
    case PST_ABSENT: return ChanRes{0, 0};
    case PST_ERR:    return ChanRes{0, CH_ERR};
    default:
      return d_plane_resolve(pr.dir, row, col_id, uns, want, vals, val_offs);
  }
}

/* Simple aggregates over column planes: no LDS staging; each lane loads 16 B
 * of every referenced value plane (two rows) plus the two state bytes, UNR
 * pairs in flight, grid-stride. The keep decision and the accumulate rules
 * are the scan kernels' (d_filter_keep / d_filter2_keep, per-lane i128
 * partials, d_simple_epilogue), so accumulator layout, overflow behaviour and
 * the parse-error flag are unchanged. */
template <int NAGGS, int UNR>
__global__ void __launch_bounds__(256)
k_plane_agg(ScanPlan plan, PlaneSet ps,
            const uint8_t *__restrict__ vals,
            const uint64_t *__restrict__ val_offs, uint64_t n_rows,
            SimpleAggAcc *__restrict__ simple_acc) {
  unsigned long long l_cnt[NAGGS];
  unsigned long long l_lo[NAGGS];
  long long l_hi[NAGGS];
  #pragma unroll
  for (int a = 0; a < NAGGS; a++) { l_cnt[a] = 0; l_lo[a] = 0; l_hi[a] = 0; }
  bool any_parse_err = false;

  const uint64_t n_pairs = (n_rows + 1) >> 1;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256u * UNR + threadIdx.x;
       p0 < n_pairs; p0 += step) {
    /* all loads first (clamped, unconditional per channel), then the rows */
    longlong2 fv[UNR], f2v[UNR], av[NAGGS][UNR];
    uint16_t fs[UNR], f2s[UNR], ast[NAGGS][UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_pairs - 1);
      fv[u] = make_longlong2(0, 0); fs[u] = 0;
      f2v[u] = make_longlong2(0, 0); f2s[u] = 0;
      if (ps.f.val) {
        fv[u] = ((const longlong2 *)ps.f.val)[p];
        fs[u] = ((const uint16_t *)ps.f.st)[p];
      }
      if (ps.f2.val) {
        f2v[u] = ((const longlong2 *)ps.f2.val)[p];
        f2s[u] = ((const uint16_t *)ps.f2.st)[p];
      }
      #pragma unroll
      for (int a = 0; a < NAGGS; a++) {
        av[a][u] = make_longlong2(0, 0); ast[a][u] = 0;
        if (ps.a[a].val) {
          av[a][u] = ((const longlong2 *)ps.a[a].val)[p];
          ast[a][u] = ((const uint16_t *)ps.a[a].st)[p];
        }
      }
    }
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = p0 + (uint64_t)u * 256u;
      #pragma unroll
      for (int h = 0; h < 2; h++) {
        uint64_t row = p * 2 + h;
        if (p >= n_pairs || row >= n_rows) continue;
        ChanRes f{0, 0}, f2{0, 0}, ag[NAGGS];
        if (ps.f.val)
          f = d_plane_chan(ps.f, (fs[u] >> (8 * h)) & 0xFFu,
                           h ? fv[u].y : fv[u].x, row, plan.filter_col_id,
                           plan.filter_col_unsigned != 0,
                           plan.filter_is_real ? 1 : 0, vals, val_offs);
        if (ps.f2.val)
          f2 = d_plane_chan(ps.f2, (f2s[u] >> (8 * h)) & 0xFFu,
                            h ? f2v[u].y : f2v[u].x, row, plan.filter2_col_id,
                            plan.filter2_col_unsigned != 0,
                            plan.filter2_is_real ? 1 : 0, vals, val_offs);
        uint32_t fl_or = f.fl | f2.fl;
        #pragma unroll
        for (int a = 0; a < NAGGS; a++) {
          ag[a] = ChanRes{0, 0};
          if (ps.a[a].val)
            ag[a] = d_plane_chan(ps.a[a], (ast[a][u] >> (8 * h)) & 0xFFu,
                                 h ? av[a][u].y : av[a][u].x, row,
                                 plan.aggs[a].col_id,
                                 plan.aggs[a].col_unsigned != 0,
                                 plan.aggs[a].kind == DAGG_COUNT_COL ? 3 : 2,
                                 vals, val_offs);
          fl_or |= ag[a].fl;
        }
        /* a parse error on any referenced column fails the request whether
           or not the filter keeps the row, as in the scan kernels */
        if (fl_or & CH_ERR) { any_parse_err = true; continue; }
        if (!(d_filter_keep(plan, (f.fl & CH_FOUND) != 0,
                            (f.fl & CH_NULL) != 0, f.v) &&
              d_filter2_keep(plan, (f2.fl & CH_FOUND) != 0,
                             (f2.fl & CH_NULL) != 0, f2.v)))
          continue;
        #pragma unroll
        for (int a = 0; a < NAGGS; a++) {
          const int32_t kind = plan.aggs[a].kind;
          if (kind == DAGG_COUNT_ROWS) { l_cnt[a]++; continue; }
          if ((ag[a].fl & (CH_FOUND | CH_NULL)) != CH_FOUND) continue;
          l_cnt[a]++;
          const int64_t v = ag[a].v;
          if (kind == DAGG_SUM_INT) {
            unsigned long long old = l_lo[a];
            unsigned long long nv = old + (unsigned long long)v;
            l_hi[a] += (nv < old ? 1 : 0) + (v < 0 ? -1 : 0);
            l_lo[a] = nv;
          } else if (kind == DAGG_MAX_INT || kind == DAGG_MIN_INT) {
            unsigned long long b =
                d_fold_xform(kind, v, plan.aggs[a].col_unsigned);
            l_lo[a] = l_lo[a] > b ? l_lo[a] : b;
          }
        }
      }
    }
  }

  d_simple_epilogue<NAGGS>(plan, simple_acc, l_cnt, l_lo, l_hi);
  if (any_parse_err)
    atomicOr((unsigned int *)&simple_acc[COPR_MAX_AGGS].cnt, 1u);
}

/* k_plane_agg specialised for one same-signedness int filter + count(*) over
 * a plane without ROWPARSE rows — the cfg2 shape, as FASTFC is to the pipe
 * kernel. The generic kernel spends ~100 instructions per row on the
 * plan-driven compare and runs issue-bound; here the host folds comparer,
 * signedness and constant into one biased unsigned range test
 *   keep = (((v ^ bias) - lo) <= span) != invert
 * so the row loop is a handful of VALU ops and the kernel follows the
 * loads. Same results: NULL never keeps, ABSENT takes the request's default
 * fill (keep_absent, decided on the host with the same test), REAL and ERR
 * cells raise the parse-error flag. PlaneFcArgs and the fold itself live in
 * plane_fold.h. */

__global__ void __launch_bounds__(256)
k_plane_fc(PlaneFcArgs fa, const longlong2 *__restrict__ val,
           const uint16_t *__restrict__ st, uint64_t n_rows,
           SimpleAggAcc *__restrict__ simple_acc) {
  constexpr int UNR = 4;
  unsigned long long cnt = 0;
  uint32_t bad = 0;
  const uint64_t n_pairs = (n_rows + 1) >> 1;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256u * UNR + threadIdx.x;
       p0 < n_pairs; p0 += step) {
    longlong2 v[UNR];
    uint32_t s[UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_pairs - 1);
      v[u] = val[p];
      s[u] = st[p];
    }
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = p0 + (uint64_t)u * 256u;
      #pragma unroll
      for (int h = 0; h < 2; h++) {
        bool live = p < n_pairs && p * 2 + h < n_rows;
        uint32_t sb = (s[u] >> (8 * h)) & 0xFFu;
        unsigned long long key =
            (unsigned long long)(h ? v[u].y : v[u].x) ^ fa.bias;
        bool k_int = ((key - fa.lo) <= fa.span) != (fa.invert != 0);
        bool keep = sb == PST_INT ? k_int
                                  : (sb == PST_ABSENT && fa.keep_absent != 0);
        cnt += (live && keep) ? 1ull : 0ull;
        bad |= (live && (sb == PST_REAL || sb >= PST_ROWPARSE)) ? 1u : 0u;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    cnt += (unsigned long long)__shfl_down((long long)cnt, off, 64);
  if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&simple_acc[0].cnt, cnt);
  if (bad) atomicOr((unsigned int *)&simple_acc[COPR_MAX_AGGS].cnt, 1u);
}

/* fold the plan's filter into k_plane_fc's range test; false = the plan or
   the plane does not fit the specialisation */
static bool plane_fc_args(const ScanPlan &plan, const PlaneSet &ps,
                          PlaneFcArgs *fa) {
  if (plan.n_aggs != 1 || plan.aggs[0].kind != DAGG_COUNT_ROWS ||
      !plan.has_filter || !ps.f.val || ps.f2.val || plan.filter2_on ||
      plan.filter_is_real || plan.filter_decode_only ||
      (plan.filter_col_unsigned != 0) != (plan.filter_const_unsigned != 0) ||
      ps.f.n_rowparse)
    return false;
  plane_fc_fold(plan.filter_cmp, plan.filter_const,
                plan.filter_col_unsigned != 0, plan.filter_const_null != 0,
                plan.filter_missing_null != 0, plan.filter_missing_val, fa);
  return true;
}

bool dev_plane_fc_shape(const ScanPlan &plan, const PlaneSet &ps,
                        PlaneFcArgs *fa) {
  return plane_fc_args(plan, ps, fa);
}

int dev_plane_agg_launch(const ScanPlan &plan, const PlaneSet &ps,
                         const DevRegion &rgn, SimpleAggAcc *d_simple,
                         void *stream) {
  if (!rgn.n_kv) return 0;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t n_pairs = (rgn.n_kv + 1) >> 1;
  PlaneFcArgs fa;
  if (plane_fc_args(plan, ps, &fa)) {
    uint64_t nb = (n_pairs + 256u * 4 - 1) / (256u * 4);
    uint32_t grid = (uint32_t)(nb < 4096 ? nb : 4096);
    hipLaunchKernelGGL(k_plane_fc, dim3(grid), dim3(256), 0, s, fa,
                       (const longlong2 *)ps.f.val,
                       (const uint16_t *)ps.f.st, rgn.n_kv, d_simple);
    return (int)hipGetLastError();
  }
  #define CASE(N, U)                                                         \
    {                                                                        \
      uint64_t nb = (n_pairs + 256u * U - 1) / (256u * U);                   \
      uint32_t grid = (uint32_t)(nb < 2048 ? nb : 2048);                     \
      hipLaunchKernelGGL((k_plane_agg<N, U>), dim3(grid), dim3(256), 0, s,   \
                         plan, ps, rgn.d_vals, rgn.d_val_offs, rgn.n_kv,     \
                         d_simple);                                          \
    }
  switch (plan.n_aggs) {
    case 1: CASE(1, 4); break;
    case 2: CASE(2, 2); break;
    case 3: CASE(3, 2); break;
    case 4: CASE(4, 2); break;
    default: CASE(COPR_MAX_AGGS, 1); break;
  }
  #undef CASE
  return (int)hipGetLastError();
}

/* ---------------- hash aggregation over column planes -------- */

/* sum(decimal) channel: what AggColView carries for the column. CH_DEC = v is
 * the cell's scaled value (an i128 for a 19..38-digit cell, CH_WIDE) with
 * frac digits; CH_BADTYPE = a non-NULL cell that holds no decimal, or a wide
 * payload that does not parse: the scan kernels fail those at the contribute
 * site, that is only when the row is kept. */
enum { CH_DEC = 8, CH_WIDE = 16, CH_BADTYPE = 32 };
struct DecRes { __int128 v; uint32_t fl; int32_t frac; };

/* decimal want of d_plane_resolve: ROWPARSE rows of a sum(decimal) column
 * (wide decimals, row-v2 rows, cells of another type) from the row bytes.
 * Kept apart from the int/real resolver so that k_plane_agg's code does not
 * change. Row-v2 cells parse as in d_v2_collect: a payload that is no
 * <= 18-digit decimal fails the request. */
__device__ __noinline__ static DecRes d_plane_resolve_dec(
    const uint8_t *dirp, uint64_t row, int64_t col_id,
    const uint8_t *vals, const uint64_t *val_offs) {
  DecRes dr{0, 0, 0};
  uint64_t o0 = val_offs[row], o1 = val_offs[row + 1];
  const uint8_t *vp = vals + o0;
  uint32_t vlen = (uint32_t)(o1 - o0);
  uint32_t dir8 = dirp ? (uint32_t)dirp[row] : 0xFEu;
  CellView cell;
  int loc = d_col_locate(vp, vlen, dir8, col_id, &cell);
  if (loc == LOC_ERR) {
    dr.fl = CH_ERR;
  } else if (loc == LOC_V2) {
    V2Row r;
    uint32_t s, e;
    if (!d_v2_parse(vp, vlen, &r)) { dr.fl = CH_ERR; return dr; }
    int fs = d_v2_find(r, col_id, &s, &e);
    if (fs < 0) return dr;
    dr.fl = CH_FOUND;
    if (fs == 0) { dr.fl |= CH_NULL; return dr; }
    int64_t sc;
    if (!d_decimal_scaled(r.vals + s, e - s, &sc, &dr.frac)) {
      dr.fl |= CH_ERR;
      return dr;
    }
    dr.v = sc;
    dr.fl |= CH_DEC;
  } else if (loc == LOC_CELL) {
    dr.fl = CH_FOUND;
    if (cell.is_null) {
      dr.fl |= CH_NULL;
    } else if (cell.has_dec) {
      dr.v = cell.dscaled; dr.frac = cell.dfrac; dr.fl |= CH_DEC;
    } else if (cell.dwide) {
      dr.fl |= CH_WIDE;
      if (d_decimal_scaled128(cell.dwide, cell.dwide_rem, &dr.v, &dr.frac))
        dr.fl |= CH_DEC;
      else
        dr.fl |= CH_BADTYPE;
    } else if (cell.has_int || cell.has_real) {
      dr.fl |= CH_BADTYPE;
    } else {
      dr.fl |= CH_ERR;
    }
  }
  return dr;
}

__device__ static inline DecRes d_plane_dec_chan(
    const PlaneRef &pr, uint32_t st, int64_t pv, uint64_t row, int64_t col_id,
    const uint8_t *vals, const uint64_t *val_offs) {
  if (st >= PST_DEC0)
    return DecRes{(__int128)pv, CH_FOUND | CH_DEC, (int32_t)(st - PST_DEC0)};
  switch (st) {
    case PST_INT:
    case PST_REAL:   return DecRes{0, CH_FOUND | CH_BADTYPE, 0};
    case PST_NULL:   return DecRes{0, CH_FOUND | CH_NULL, 0};
    case PST_ABSENT: return DecRes{0, 0, 0};
    case PST_ERR:    return DecRes{0, CH_ERR, 0};
    default:
      return d_plane_resolve_dec(pr.dir, row, col_id, vals, val_offs);
  }
}

/* FastHashAgg (int group key) over column planes. Loads as in k_plane_agg:
 * per lane 16 B (two rows) of every distinct referenced value plane plus the
 * two state bytes, UNR pairs issued before any row work, tail pairs clamped
 * into the planes' slack. The keep decision is d_filter_keep /
 * d_filter2_keep; slot selection, accumulation and the flush are the helpers
 * above. Parse errors: a PST_ERR row or a failed ROWPARSE resolve raises
 * ht.error[1] whether or not the row is kept; sum(decimal) scaling errors and
 * type mismatches only for a kept row. The grid is capped by the host so the
 * number of LDS-table flushes stays bounded. Dynamic LDS: lslots keys, then
 * lslots * n_aggs accumulators. NAGGS >= n_aggs is the unroll bound only:
 * every accumulator array keeps the plan's n_aggs stride. */
template <int NAGGS, int UNR>
__global__ void __launch_bounds__(256)
k_plane_hash(ScanPlan plan, PlaneSet ps, HashAggTable ht,
             const uint8_t *__restrict__ vals,
             const uint64_t *__restrict__ val_offs, uint64_t n_rows) {
  extern __shared__ __align__(16) uint8_t lds[];
  const uint32_t LSLOTS = plan.lds_agg_slots;
  long long *lkeys = (long long *)lds;
  SimpleAggAcc *laccs = (SimpleAggAcc *)(lkeys + LSLOTS);
  const uint32_t na = min((uint32_t)plan.n_aggs, (uint32_t)NAGGS);
  d_hash_lds_init<NAGGS>(plan, lkeys, laccs, LSLOTS);
  __syncthreads();
  bool any_parse_err = false;

  const uint64_t n_pairs = (n_rows + 1) >> 1;
  const uint64_t step = (uint64_t)gridDim.x * 256u * UNR;
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256u * UNR + threadIdx.x;
       p0 < n_pairs; p0 += step) {
    /* all loads first (clamped, unconditional per distinct plane) */
    longlong2 gv[UNR], fv[UNR], f2v[UNR], av[NAGGS][UNR];
    uint16_t gs[UNR], fs[UNR], f2s[UNR], ast[NAGGS][UNR];
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = min(p0 + (uint64_t)u * 256u, n_pairs - 1);
      gv[u] = ((const longlong2 *)ps.g.val)[p];
      gs[u] = ((const uint16_t *)ps.g.st)[p];
      fv[u] = make_longlong2(0, 0); fs[u] = 0;
      f2v[u] = make_longlong2(0, 0); f2s[u] = 0;
      if (ps.f.val) {
        fv[u] = ((const longlong2 *)ps.f.val)[p];
        fs[u] = ((const uint16_t *)ps.f.st)[p];
      }
      if (ps.f2.val) {
        f2v[u] = ((const longlong2 *)ps.f2.val)[p];
        f2s[u] = ((const uint16_t *)ps.f2.st)[p];
      }
      #pragma unroll
      for (int a = 0; a < NAGGS; a++) {
        av[a][u] = make_longlong2(0, 0); ast[a][u] = 0;
        if (ps.a[a].val && ps.a_src[a] == 0) {
          av[a][u] = ((const longlong2 *)ps.a[a].val)[p];
          ast[a][u] = ((const uint16_t *)ps.a[a].st)[p];
        }
      }
    }
    /* a column referenced twice was loaded once: copy the registers */
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      #pragma unroll
      for (int a = 0; a < NAGGS; a++) {
        const int32_t src = ps.a_src[a];
        if (src == 1) { av[a][u] = gv[u]; ast[a][u] = gs[u]; }
        else if (src == 2) { av[a][u] = fv[u]; ast[a][u] = fs[u]; }
        else if (src == 3) { av[a][u] = f2v[u]; ast[a][u] = f2s[u]; }
        #pragma unroll
        for (int b = 0; b < a; b++)
          if (src == 4 + b) { av[a][u] = av[b][u]; ast[a][u] = ast[b][u]; }
      }
    }
    #pragma unroll
    for (int u = 0; u < UNR; u++) {
      uint64_t p = p0 + (uint64_t)u * 256u;
      #pragma unroll
      for (int h = 0; h < 2; h++) {
        uint64_t row = p * 2 + h;
        if (p >= n_pairs || row >= n_rows) continue;
        ChanRes f{0, 0}, f2{0, 0}, ag[NAGGS];
        DecRes dg[NAGGS];
        ChanRes g = d_plane_chan(ps.g, (gs[u] >> (8 * h)) & 0xFFu,
                                 h ? gv[u].y : gv[u].x, row, plan.group_col_id,
                                 plan.group_col_unsigned != 0, 0, vals,
                                 val_offs);
        if (ps.f.val)
          f = d_plane_chan(ps.f, (fs[u] >> (8 * h)) & 0xFFu,
                           h ? fv[u].y : fv[u].x, row, plan.filter_col_id,
                           plan.filter_col_unsigned != 0,
                           plan.filter_is_real ? 1 : 0, vals, val_offs);
        if (ps.f2.val)
          f2 = d_plane_chan(ps.f2, (f2s[u] >> (8 * h)) & 0xFFu,
                            h ? f2v[u].y : f2v[u].x, row, plan.filter2_col_id,
                            plan.filter2_col_unsigned != 0,
                            plan.filter2_is_real ? 1 : 0, vals, val_offs);
        uint32_t fl_or = g.fl | f.fl | f2.fl;
        #pragma unroll
        for (int a = 0; a < NAGGS; a++) {
          ag[a] = ChanRes{0, 0};
          dg[a] = DecRes{0, 0, 0};
          if (ps.a[a].val) {
            const uint32_t st = (ast[a][u] >> (8 * h)) & 0xFFu;
            const int64_t pv = h ? av[a][u].y : av[a][u].x;
            if (plan.aggs[a].kind == DAGG_SUM_DEC) {
              dg[a] = d_plane_dec_chan(ps.a[a], st, pv, row,
                                       plan.aggs[a].col_id, vals, val_offs);
              ag[a].fl = dg[a].fl;
            } else {
              ag[a] = d_plane_chan(ps.a[a], st, pv, row, plan.aggs[a].col_id,
                                   plan.aggs[a].col_unsigned != 0,
                                   plan.aggs[a].kind == DAGG_COUNT_COL ? 3 : 2,
                                   vals, val_offs);
            }
          }
          fl_or |= ag[a].fl;
        }
        if (fl_or & CH_ERR) { any_parse_err = true; continue; }
        if (!(d_filter_keep(plan, (f.fl & CH_FOUND) != 0,
                            (f.fl & CH_NULL) != 0, f.v) &&
              d_filter2_keep(plan, (f2.fl & CH_FOUND) != 0,
                             (f2.fl & CH_NULL) != 0, f2.v)))
          continue;
        const bool row_wide = d_row_wide<NAGGS>(plan, [&](int a) {
          return DecIn{(ag[a].fl & (CH_FOUND | CH_NULL)) == CH_FOUND,
                       (ag[a].fl & CH_WIDE) != 0, (ag[a].fl & CH_DEC) != 0,
                       (int64_t)dg[a].v, dg[a].frac};
        });
        HashSlot hs = d_hash_row_slot(
            ht, plan.table_size, na, (g.fl & CH_FOUND) != 0,
            (g.fl & CH_NULL) != 0, g.v, row_wide, lkeys, laccs, LSLOTS);
        #pragma unroll
        for (int a = 0; a < NAGGS; a++) {
          const DevAggSpec &sp = plan.aggs[a];
          bool dec_wide = false;       /* value does not fit a scaled i64 */
          __int128 vw = 0;
          int64_t v = 0;
          if ((uint32_t)a >= na) continue;
          if (sp.kind != DAGG_COUNT_ROWS) {
            if ((ag[a].fl & (CH_FOUND | CH_NULL)) != CH_FOUND) continue;
            if (sp.kind == DAGG_SUM_DEC) {
              if (!(ag[a].fl & CH_DEC) ||
                  !d_dec_rescale(dg[a].v, dg[a].frac, sp.target_frac, &v, &vw,
                                 &dec_wide)) {
                any_parse_err = true;   /* bad type, or > 38 digits */
                continue;
              }
            } else {
              v = ag[a].v;
            }
          }
          if (hs.acc &&
              !d_hash_update<true>(sp, hs.acc + a,
                                   hs.ext ? hs.ext + a * 2 : nullptr, v, vw,
                                   dec_wide))
            any_parse_err = true;     /* no ext buffers: loud */
        }
      }
    }
  }

  if (LSLOTS) {
    __syncthreads();
    d_hash_lds_flush<NAGGS, true>(plan, ht, lkeys, laccs, LSLOTS);
  }
  if (any_parse_err) atomicOr(ht.error + 1, 1u);
}

int dev_plane_hash_launch(const ScanPlan &plan, const PlaneSet &ps,
                          const DevRegion &rgn, const HashAggTable &ht,
                          void *stream) {
  if (!rgn.n_kv) return 0;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t n_pairs = (rgn.n_kv + 1) >> 1;
  const uint32_t lds_b =
      plan.lds_agg_slots *
      (8u + (uint32_t)plan.n_aggs * (uint32_t)sizeof(SimpleAggAcc));
  /* every block flushes its LDS table once: cap the grid at what the device
     keeps resident at 256 CUs x 8 blocks, and let the blocks stride */
  #define CASE(N, U)                                                         \
    {                                                                        \
      uint64_t nb = (n_pairs + 256u * U - 1) / (256u * U);                   \
      uint32_t grid = (uint32_t)(nb < 2048 ? nb : 2048);                     \
      hipLaunchKernelGGL((k_plane_hash<N, U>), dim3(grid), dim3(256), lds_b, \
                         s, plan, ps, ht, rgn.d_vals, rgn.d_val_offs,        \
                         rgn.n_kv);                                          \
    }
  switch (plan.n_aggs) {
    case 1: CASE(1, 2); break;
    case 2: CASE(2, 2); break;
    case 3: CASE(3, 2); break;
    case 4: CASE(4, 2); break;
    default: CASE(COPR_MAX_AGGS, 1); break;
  }
  #undef CASE
  return (int)hipGetLastError();
}

/* ---------------- project kernel (row-returning scans) ----------------
 * Not the hot path: dynamic out-column indexing may spill; correctness and
 * byte-identical output shape are what matter here. */
__global__ void __launch_bounds__(THREADS)
k_scan_project(ScanPlan plan,
               const uint8_t *__restrict__ vals, const uint64_t *__restrict__ val_offs,
               const uint8_t *__restrict__ keys, const uint64_t *__restrict__ key_offs,
               uint64_t n_rows, ProjectOut po) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t rpt = plan.rows_per_tile;
  const uint64_t n_tiles = (n_rows + rpt - 1) / rpt;
  bool any_parse_err = false;

  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    uint64_t gbase = val_offs[row0];
    uint32_t tlen = (uint32_t)(val_offs[row1] - gbase);
    __syncthreads();
    uint32_t shift = stage_tile(vals, gbase, tlen, lds);

    for (uint64_t my_row = row0 + threadIdx.x; my_row < row1; my_row += blockDim.x) {
      const uint8_t *vp = lds + shift + (uint32_t)(val_offs[my_row] - gbase);
      uint32_t vlen = (uint32_t)(val_offs[my_row + 1] - val_offs[my_row]);
      bool parse_ok = true;
      bool filt_found = false, filt_null = false; int64_t filt_v = 0;
      bool d2_found = false, d2_null = false;
      int64_t d2_v = 0;
      int64_t idx_handle = 0;
      unsigned long long cell_pack[COPR_MAX_OUT_COLS];
      for (int j = 0; j < plan.n_out; j++) cell_pack[j] = 0xFFFFFull;
      int needed = (plan.has_filter ? 1 : 0) + (plan.dec2_col_id ? 1 : 0) +
                   plan.n_out;
      int found = 0;

      if (plan.index_mode) {
        /* index project: vp IS the index key (the launcher streams the key
           stream); out cols are POSITIONAL raw datum spans in the key
           (extract_columns_from_datum_format :504-517); the handle comes
           from the trailing key datum or the value
           (d_index_value_split). V4 restore-data rows are not native in
           project mode (columns would live in the value's row-v2). */
        if (vlen < 19 || vp[0] != 't' || vp[9] != '_' || vp[10] != 'i') {
          parse_ok = false;
        } else {
          bool hfound = false;
          uint32_t pos = 19;
          int64_t ci = 0;
          while (pos < vlen && parse_ok) {
            CellView cell;
            d_parse_datum(vp + pos, vlen - pos, &cell);
            if (!cell.len) { parse_ok = false; break; }
            if (ci == (int64_t)plan.index_n_cols) {
              if (!cell.has_int) { parse_ok = false; break; }
              idx_handle = cell.ival;
              hfound = true;
            }
            for (int j = 0; j < plan.n_out; j++) {
              if (plan.out_is_handle[j]) continue;
              if (plan.out_col_ids[j] == ci) {
                uint64_t goff = val_offs[my_row] + pos;
                if (cell.len >= 0xFFFFEu) { parse_ok = false; break; }
                cell_pack[j] = (goff << 20) | cell.len;
              }
            }
            if (plan.has_filter && !filt_found && ci == plan.filter_col_id) {
              filt_found = true;
              if (cell.is_null) filt_null = true;
              else if (cell.has_int) filt_v = cell.ival;
              else parse_ok = false;
            }
            if (plan.dec2_col_id && !d2_found && ci == plan.dec2_col_id) {
              d2_found = true;
              if (cell.is_null) d2_null = true;
              else if (cell.has_int) d2_v = cell.ival;
              else parse_ok = false;
            }
            pos += cell.len;
            ci++;
          }
          if (parse_ok && !hfound && plan.aux_vals) {
            uint64_t o0 = plan.aux_val_offs[my_row];
            uint64_t o1 = plan.aux_val_offs[my_row + 1];
            int64_t vh = 0;
            bool has_h = false;
            const uint8_t *restore = nullptr;
            uint32_t rl = 0;
            if (!d_index_value_split(plan.aux_vals + o0, (uint32_t)(o1 - o0),
                                     &vh, &has_h, &restore, &rl) ||
                restore)
              parse_ok = false;
            else if (has_h) {
              idx_handle = vh;
              hfound = true;
            }
          }
          bool need_handle = false;
          for (int j = 0; j < plan.n_out; j++)
            if (plan.out_is_handle[j]) need_handle = true;
          if (parse_ok && need_handle && !hfound) parse_ok = false;
        }
      } else
      if (vlen > 1 && vp[0] == 128) {
        /* row v2: direct column lookup; value cells are RAW payloads, the
           host re-encodes them as datums (compat_v1.rs:28-126). 0xFFFFE
           marks an explicit NULL cell (v1 NULLs are 1-byte datums with a
           capturable span; v2 NULLs have no bytes). */
        V2Row r2;
        if (!d_v2_parse(vp, vlen, &r2)) {
          parse_ok = false;
        } else {
          if (plan.has_filter) {
            uint32_t s2, e2;
            int vst = d_v2_find(r2, plan.filter_col_id, &s2, &e2);
            if (vst >= 0) {
              filt_found = true;
              if (vst == 0) filt_null = true;
              else if (!d_v2_int(r2.vals + s2, e2 - s2,
                                 plan.filter_col_unsigned, &filt_v))
                parse_ok = false;
            }
          }
          if (plan.dec2_col_id) {
            uint32_t s2, e2;
            int vst = d_v2_find(r2, plan.dec2_col_id, &s2, &e2);
            if (vst >= 0) {
              d2_found = true;
              if (vst == 0) d2_null = true;
              else if (!d_v2_int(r2.vals + s2, e2 - s2,
                                 plan.dec2_col_unsigned, &d2_v))
                parse_ok = false;
            }
          }
          for (int j = 0; j < plan.n_out && parse_ok; j++) {
            if (plan.out_is_handle[j]) continue;
            uint32_t s2, e2;
            int vst = d_v2_find(r2, plan.out_col_ids[j], &s2, &e2);
            if (vst < 0) continue;                 /* missing: default fill */
            if (vst == 0) { cell_pack[j] = 0xFFFFEull; continue; }
            uint64_t goff = val_offs[my_row] + (uint32_t)(r2.vals + s2 - vp);
            uint32_t clen = e2 - s2;
            if (clen >= 0xFFFFEu) { parse_ok = false; break; }
            cell_pack[j] = (goff << 20) | clen;
          }
        }
      } else {
      ROW_FOREACH_BEGIN(vp, vlen)
        if (plan.has_filter && !filt_found && cell_id == plan.filter_col_id) {
          filt_found = true;
          if (cell.is_null) filt_null = true;
          else if (plan.filter_is_real ? cell.has_real : cell.has_int) filt_v = cell.ival;
          else parse_ok = false;
          found++;
        }
        if (plan.dec2_col_id && !d2_found && cell_id == plan.dec2_col_id) {
          d2_found = true;
          if (cell.is_null) d2_null = true;
          else if (cell.has_int) d2_v = cell.ival;
          else parse_ok = false;
          found++;
        }
        for (int j = 0; j < plan.n_out; j++) {
          if (plan.out_is_handle[j] || cell_pack[j] != 0xFFFFFull) continue;
          if (cell_id == plan.out_col_ids[j]) {
            uint64_t goff = val_offs[my_row] + cell_off;
            cell_pack[j] = (goff << 20) | (cell.len & 0xFFFFFu);
            found++;
          }
        }
        if (found >= needed) break;
      ROW_FOREACH_END()
      }

      if (!parse_ok) {
        any_parse_err = true;
      } else {
        bool kerr = false;
        bool keep = d_keep2(plan, filt_found, filt_null, filt_v, d2_found,
                            d2_null, d2_v, &kerr);
        if (kerr) { any_parse_err = true; keep = false; }
        po.keep[my_row] = keep ? 1 : 0;
        if (plan.has_filter && po.filt_vals) {
          po.filt_vals[my_row] = filt_v;
          po.filt_state[my_row] = !filt_found ? 2 : (filt_null ? 1 : 0);
        }
        if (plan.dec2_col_id && po.dec2_vals) {
          po.dec2_vals[my_row] = d2_v;
          po.dec2_state[my_row] = !d2_found ? 2 : (d2_null ? 1 : 0);
        }
        if (keep) {
          for (int j = 0; j < plan.n_out; j++) {
            if (plan.out_is_handle[j]) {
              if (plan.index_mode) {
                po.handles[my_row] = idx_handle;
              } else {
                const uint8_t *kp = keys + key_offs[my_row];
                uint64_t h = d_be_u64(kp + 11) ^ 0x8000000000000000ull;
                po.handles[my_row] = (long long)h;
              }
            } else {
              po.cells[my_row * plan.n_out + j] = cell_pack[j];
            }
          }
        }
      }
    }
  }
  if (any_parse_err) atomicOr(po.error + 1, 1u);
}

/* ---------------- CRC-64/XZ kernel (checksum.rs:105-114) ----------------
 * Per-KV digest over key||value, XOR-fold per wave then one atomicXor per
 * block (the running XOR is order-independent, checksum.rs:78-87).
 *
 * k_crc64_reg: one lane per KV, row bytes loaded from GLOBAL
 * memory into 8xu64 register chunks — no tile staging, no barriers. LDS
 * holds only the 16 KiB slice-by-8 tables, so 8 blocks/CU keep 8 waves/SIMD
 * of independent CRC chains in flight. The r01 tiled kernel measured 80%
 * SQ_WAIT_ANY (wave-parked) at 3 blocks/CU: the per-lane chain of
 * LDS-window + 8 table reads per 8 bytes has ~50-cycle dependent latency
 * per step and the stage/parse barrier phases serialized on top
 * (profiles/r02_cfg4_*). More independent chains per SIMD is the fix, not
 * more LDS bandwidth. The variants that lost to it (two-row interleave,
 * slice-by-16, no-prefetch, 6 waves/SIMD, the tiled kernel) are recorded in
 * DESIGN.md §9b/§10. */
/* always_inline: kept so that k_crc64_reg's code stays as measured; outlined,
 * this function cost 44 B/lane of scratch and half the CRC throughput */
__device__ __attribute__((always_inline)) static inline uint64_t
d_crc64_stream(const uint8_t *__restrict__ base, uint64_t b0, uint64_t b1,
               uint64_t crc, const uint64_t *__restrict__ tab) {
  uint64_t len = b1 - b0;
  if (!len) return crc;
  /* aligned u64 stream with a funnel shift; region buffers carry +2 KiB
     tail slack so word over-reads past b1 are in-bounds */
  const uint64_t *q = (const uint64_t *)(base + (b0 & ~7ull));
  uint32_t sh = (uint32_t)(b0 & 7) * 8u;
  uint64_t prev = q[0];
  uint64_t wi = 1;
  uint64_t n8 = len >> 3;
  auto step8 = [&](uint64_t cur) {
    crc ^= cur;
    crc = tab[7 * 256 + (uint32_t)(crc & 0xFF)] ^
          tab[6 * 256 + (uint32_t)((crc >> 8) & 0xFF)] ^
          tab[5 * 256 + (uint32_t)((crc >> 16) & 0xFF)] ^
          tab[4 * 256 + (uint32_t)((crc >> 24) & 0xFF)] ^
          tab[3 * 256 + (uint32_t)((crc >> 32) & 0xFF)] ^
          tab[2 * 256 + (uint32_t)((crc >> 40) & 0xFF)] ^
          tab[1 * 256 + (uint32_t)((crc >> 48) & 0xFF)] ^
          tab[0 * 256 + (uint32_t)(crc >> 56)];
  };
  if (n8 >= 8) {
    /* software pipeline over 64-byte register chunks: chunk k+1's 8
       independent loads are in flight while the dependent table chain
       consumes chunk k (the unpipelined form measured 54% SQ_WAIT_ANY —
       one HBM latency exposed per chunk). Costs ~32 VGPRs: pair with
       __launch_bounds__(256, 4), NOT 8 (at 8 it spills 52 B/lane). */
    uint64_t w[8];
    #pragma unroll
    for (int j = 0; j < 8; j++) w[j] = q[wi + j];
    wi += 8;
    n8 -= 8;
    while (n8 >= 8) {
      uint64_t w2[8];
      #pragma unroll
      for (int j = 0; j < 8; j++) w2[j] = q[wi + j];
      #pragma unroll
      for (int j = 0; j < 8; j++) {
        uint64_t cur = sh ? ((prev >> sh) | (w[j] << (64 - sh))) : prev;
        prev = w[j];
        step8(cur);
      }
      #pragma unroll
      for (int j = 0; j < 8; j++) w[j] = w2[j];
      wi += 8;
      n8 -= 8;
    }
    #pragma unroll
    for (int j = 0; j < 8; j++) {
      uint64_t cur = sh ? ((prev >> sh) | (w[j] << (64 - sh))) : prev;
      prev = w[j];
      step8(cur);
    }
  }
  while (n8) {
    uint64_t w = q[wi++];
    uint64_t cur = sh ? ((prev >> sh) | (w << (64 - sh))) : prev;
    prev = w;
    step8(cur);
    n8--;
  }
  uint32_t tail = (uint32_t)(len & 7u);
  if (tail) {
    uint64_t w = q[wi];
    uint64_t cur = sh ? ((prev >> sh) | (w << (64 - sh))) : prev;
    for (uint32_t t = 0; t < tail; t++) {
      crc = tab[(uint32_t)((crc ^ cur) & 0xFF)] ^ (crc >> 8);
      cur >>= 8;
    }
  }
  return crc;
}

/* 4 waves/SIMD (128 VGPRs, no spill): d_crc64_stream's software pipeline
 * hides the per-chunk HBM latency inside the lane */
__global__ void __launch_bounds__(THREADS, 4)
k_crc64_reg(const uint8_t *__restrict__ vals,
            const uint64_t *__restrict__ val_offs,
            const uint8_t *__restrict__ keys,
            const uint64_t *__restrict__ key_offs, uint64_t n_rows,
            const uint64_t *__restrict__ g_tables,
            unsigned long long *__restrict__ out_xor) {
  __shared__ uint64_t tab[8 * 256];
  for (uint32_t i = threadIdx.x; i < 8 * 256u; i += blockDim.x)
    tab[i] = g_tables[i];
  __syncthreads();
  unsigned long long acc = 0;
  for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < n_rows; row += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t crc = ~0ull;
    crc = d_crc64_stream(keys, key_offs[row], key_offs[row + 1], crc, tab);
    crc = d_crc64_stream(vals, val_offs[row], val_offs[row + 1], crc, tab);
    acc ^= ~crc;
  }
  for (int off = 32; off > 0; off >>= 1)
    acc ^= (unsigned long long)__shfl_down((long long)acc, off, 64);
  if ((threadIdx.x & 63u) == 0 && acc) atomicXor(out_xor, acc);
}

/* ---------------- MVCC write-CF version filter ----------------
 * Input: sorted write-CF entries (user-key asc, commit_ts desc):
 *   key   = memcomparable(user_key) || BE(~commit_ts)  (types.rs:152-161)
 *   value = [type][varint start_ts][tags 'v','R','F','l','S']
 *            (write.rs:296-361)
 * Output: the visible (raw user_key, short_value) stream — exactly what
 * TikvStorage hands the scan executors (storage_impl.rs:93).
 * Rule (forward.rs:440-515): newest version with commit_ts <= read_ts; a
 * gc fence in (0, read_ts] makes the key invisible (write.rs:425-442);
 * Put -> emit short value (default-CF lookup unsupported: error),
 * Delete -> skip key, Lock/Rollback -> older version unless
 * LastChange::NotExist (types.rs:721-731). */
__device__ static inline bool d_parse_write_rec(const uint8_t *v, uint32_t len,
                                                char *type, uint32_t *sv_off,
                                                uint32_t *sv_len,
                                                uint64_t *fence, int *lc_ne,
                                                uint64_t *start_ts = nullptr) {
  *sv_off = 0; *sv_len = 0; *fence = 0; *lc_ne = 0;
  if (len < 1) return false;
  char t = (char)v[0];
  if (t != 'P' && t != 'D' && t != 'L' && t != 'R') return false;
  *type = t;
  uint32_t p = 1;
  uint64_t sts; uint32_t n;
  if (!d_var_u64(v + p, len - p, &sts, &n)) return false;
  if (start_ts) *start_ts = sts;
  p += n;
  while (p < len) {
    uint8_t tag = v[p++];
    if (tag == 'v') {
      if (p >= len) return false;
      uint8_t l = v[p++];
      if (p + l > len) return false;
      *sv_off = p; *sv_len = l;
      p += l;
    } else if (tag == 'R') {
    } else if (tag == 'F') {
      if (p + 8 > len) return false;
      *fence = d_be_u64(v + p);
      p += 8;
    } else if (tag == 'l') {
      if (p + 8 > len) return false;
      uint64_t lts = d_be_u64(v + p);
      p += 8;
      uint64_t vers; uint32_t nn;
      if (!d_var_u64(v + p, len - p, &vers, &nn)) return false;
      p += nn;
      if (lts == 0 && vers > 0) *lc_ne = 1;
    } else if (tag == 'S') {
      uint64_t vv; uint32_t nn;
      if (!d_var_u64(v + p, len - p, &vv, &nn)) return false;
      p += nn;
    } else {
      break;                                   /* unknown tag stops parse */
    }
  }
  return true;
}

__device__ static inline bool d_ukey_eq(const uint8_t *a, uint32_t alen,
                                        const uint8_t *b, uint32_t blen) {
  if (alen != blen) return false;
  uint32_t i = 0;
  for (; i + 8 <= alen; i += 8) {
    uint64_t xa, xb;
    memcpy(&xa, a + i, 8);
    memcpy(&xb, b + i, 8);
    if (xa != xb) return false;
  }
  for (; i < alen; i++)
    if (a[i] != b[i]) return false;
  return true;
}

/* lexicographic compare of (ukey||BE(~ts)) against a default-CF key */
__device__ static inline int d_dkey_cmp(const uint8_t *u, uint32_t ulen,
                                        uint64_t ts_desc_be,
                                        const uint8_t *d, uint32_t dlen) {
  uint32_t tot = ulen + 8;
  uint32_t n = tot < dlen ? tot : dlen;
  for (uint32_t i = 0; i < n; i++) {
    uint8_t ub = i < ulen ? u[i]
                          : (uint8_t)(ts_desc_be >> (8 * (7 - (i - ulen))));
    if (ub != d[i]) return ub < d[i] ? -1 : 1;
  }
  return tot == dlen ? 0 : (tot < dlen ? -1 : 1);
}

/* default-CF lookup (forward.rs:433-515 load_data_from_default_cf /
 * near_loadData; write.rs:296 short-value-vs-default split): the value of a
 * Put without a short value lives at key = memcomparable(user_key) ||
 * BE(~start_ts) in the default CF. Returns the entry index or UINT64_MAX. */
__device__ static inline uint64_t d_default_cf_find(
    const uint8_t *__restrict__ dkeys, const uint64_t *__restrict__ dko,
    uint64_t dn, const uint8_t *u, uint32_t ulen, uint64_t start_ts) {
  uint64_t ts_desc_be = ~start_ts;       /* compared as BE bytes */
  uint64_t lo = 0, hi = dn;
  while (lo < hi) {
    uint64_t mid = (lo + hi) >> 1;
    const uint8_t *d = dkeys + dko[mid];
    uint32_t dlen = (uint32_t)(dko[mid + 1] - dko[mid]);
    int c = d_dkey_cmp(u, ulen, ts_desc_be, d, dlen);
    if (c == 0) return mid;
    if (c < 0) hi = mid;
    else lo = mid + 1;
  }
  return UINT64_MAX;
}

__global__ void __launch_bounds__(THREADS)
k_mvcc_flags(const uint8_t *__restrict__ keys, const uint64_t *__restrict__ ko,
             const uint8_t *__restrict__ vals, const uint64_t *__restrict__ vo,
             uint64_t n, uint64_t read_ts,
             const uint8_t *__restrict__ dkeys,
             const uint64_t *__restrict__ dko,
             const uint64_t *__restrict__ dvo, uint64_t dn,
             uint64_t *__restrict__ dref,
             uint8_t *__restrict__ vis, uint32_t *__restrict__ ksz,
             uint32_t *__restrict__ vsz, unsigned int *__restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    vis[i] = 0; ksz[i] = 0; vsz[i] = 0;
    if (dref) dref[i] = UINT64_MAX;
    uint32_t klen = (uint32_t)(ko[i + 1] - ko[i]);
    if (klen < 17 || ((klen - 8) % 9) != 0) { atomicOr(err, 1u); continue; }
    const uint8_t *k = keys + ko[i];
    uint32_t ulen = klen - 8;
    uint64_t ts = ~d_be_u64(k + ulen);
    if (ts > read_ts) continue;
    char type; uint32_t sv_off, sv_len; uint64_t fence; int lc_ne;
    uint64_t start_ts = 0;
    if (!d_parse_write_rec(vals + vo[i], (uint32_t)(vo[i + 1] - vo[i]),
                           &type, &sv_off, &sv_len, &fence, &lc_ne,
                           &start_ts)) {
      atomicOr(err, 1u);
      continue;
    }
    if (type != 'P') continue;
    if (fence != 0 && fence <= read_ts) continue;
    /* every newer same-key version with ts <= read_ts must be a valid
       Lock/Rollback that keeps iterating */
    bool emit = true;
    for (uint64_t j = i; j-- > 0;) {
      uint32_t klj = (uint32_t)(ko[j + 1] - ko[j]);
      if (klj < 17) { atomicOr(err, 1u); emit = false; break; }
      const uint8_t *kj = keys + ko[j];
      if (!d_ukey_eq(k, ulen, kj, klj - 8)) break;
      uint64_t tsj = ~d_be_u64(kj + klj - 8);
      if (tsj > read_ts) continue;
      char tj; uint32_t so, sl; uint64_t fj; int lnj;
      if (!d_parse_write_rec(vals + vo[j], (uint32_t)(vo[j + 1] - vo[j]),
                             &tj, &so, &sl, &fj, &lnj)) {
        atomicOr(err, 1u);
        emit = false;
        break;
      }
      if (fj != 0 && fj <= read_ts) { emit = false; break; }
      if (tj != 'L' && tj != 'R') { emit = false; break; }
      if (lnj) { emit = false; break; }
    }
    if (!emit) continue;
    uint32_t out_vlen = sv_len;
    if (sv_len == 0 && sv_off == 0) {
      /* no short value: the row value lives in the default CF at
         user_key||start_ts (forward.rs:433-515; write.rs:296) */
      if (!dkeys) { atomicOr(err, 2u); continue; }   /* no stream: loud */
      uint64_t m = d_default_cf_find(dkeys, dko, dn, k, ulen, start_ts);
      if (m == UINT64_MAX) { atomicOr(err, 1u); continue; }  /* corruption */
      dref[i] = m;
      out_vlen = (uint32_t)(dvo[m + 1] - dvo[m]);
    }
    /* decoded user key length from the memcomparable groups */
    uint32_t groups = ulen / 9;
    uint8_t marker = k[ulen - 1];
    uint32_t pad = 0xFFu - marker;
    if (pad > 8) { atomicOr(err, 1u); continue; }
    vis[i] = 1;
    ksz[i] = (groups - 1) * 8 + (8 - pad);
    vsz[i] = out_vlen;
  }
}

__global__ void __launch_bounds__(THREADS)
k_mvcc_widen(const uint8_t *__restrict__ vis, const uint32_t *__restrict__ ksz,
             const uint32_t *__restrict__ vsz, uint64_t n,
             uint64_t *__restrict__ v64, uint64_t *__restrict__ k64,
             uint64_t *__restrict__ s64) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    v64[i] = vis[i];
    k64[i] = ksz[i];
    s64[i] = vsz[i];
  }
}

__global__ void __launch_bounds__(THREADS)
k_mvcc_gather(const uint8_t *__restrict__ keys, const uint64_t *__restrict__ ko,
              const uint8_t *__restrict__ vals, const uint64_t *__restrict__ vo,
              uint64_t n,
              const uint8_t *__restrict__ dvals,
              const uint64_t *__restrict__ dvo,
              const uint64_t *__restrict__ dref,
              const uint8_t *__restrict__ vis, const uint32_t *__restrict__ ksz,
              const uint32_t *__restrict__ vsz,
              const uint64_t *__restrict__ idx_sc,
              const uint64_t *__restrict__ kb_sc,
              const uint64_t *__restrict__ vb_sc,
              uint8_t *__restrict__ out_keys, uint64_t *__restrict__ out_ko,
              uint8_t *__restrict__ out_vals, uint64_t *__restrict__ out_vo,
              unsigned long long *__restrict__ max_row) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (!vis[i]) continue;
    uint64_t pos = idx_sc[i], kout = kb_sc[i], vout = vb_sc[i];
    const uint8_t *k = keys + ko[i];
    uint32_t dklen = ksz[i];
    /* memcomparable decode: strip the marker byte of each 9-byte group */
    uint32_t g = 0, w = 0;
    while (w < dklen) {
      uint32_t take = dklen - w < 8 ? dklen - w : 8;
      for (uint32_t b = 0; b < take; b++)
        out_keys[kout + w + b] = k[g * 9 + b];
      w += take;
      g++;
    }
    char type; uint32_t sv_off, sv_len; uint64_t fence; int lc_ne;
    d_parse_write_rec(vals + vo[i], (uint32_t)(vo[i + 1] - vo[i]),
                      &type, &sv_off, &sv_len, &fence, &lc_ne);
    const uint8_t *sv;
    uint32_t out_vlen;
    if (dref && dref[i] != UINT64_MAX) {     /* default-CF value */
      uint64_t m = dref[i];
      sv = dvals + dvo[m];
      out_vlen = (uint32_t)(dvo[m + 1] - dvo[m]);
    } else {
      sv = vals + vo[i] + sv_off;
      out_vlen = sv_len;
    }
    for (uint32_t b = 0; b < out_vlen; b++) out_vals[vout + b] = sv[b];
    out_ko[pos] = kout;
    out_vo[pos] = vout;
    atomicMax(max_row, (unsigned long long)out_vlen);
  }
}

int dev_mvcc_build(const uint8_t *d_keys, const uint64_t *d_ko,
                   const uint8_t *d_vals, const uint64_t *d_vo, uint64_t n,
                   const uint8_t *dd_keys, const uint64_t *dd_ko,
                   const uint8_t *dd_vals, const uint64_t *dd_vo, uint64_t dn,
                   uint64_t read_ts, DevRegion *out, int *unsupported,
                   void *stream) {
  *unsupported = 0;
  hipStream_t s = (hipStream_t)stream;
  uint8_t *vis = nullptr;
  uint32_t *ksz = nullptr, *vsz = nullptr;
  unsigned int *err = nullptr;
  uint64_t *v64 = nullptr, *k64 = nullptr, *s64 = nullptr;
  uint64_t *idx_sc = nullptr, *kb_sc = nullptr, *vb_sc = nullptr;
  uint64_t *dref = nullptr;
  unsigned long long *d_maxrow = nullptr;
  void *tmp = nullptr;
  size_t tmp_bytes = 0;
  hipError_t e = hipSuccess;
  auto freeall = [&]() {
    hipFree(vis); hipFree(ksz); hipFree(vsz); hipFree(err);
    hipFree(v64); hipFree(k64); hipFree(s64);
    hipFree(idx_sc); hipFree(kb_sc); hipFree(vb_sc);
    hipFree(dref); hipFree(d_maxrow); hipFree(tmp);
  };
  uint64_t na = n ? n : 1;
  if (e == hipSuccess) e = hipMalloc(&vis, na);
  if (e == hipSuccess) e = hipMalloc(&ksz, na * 4);
  if (e == hipSuccess) e = hipMalloc(&vsz, na * 4);
  if (e == hipSuccess) e = hipMalloc(&err, 4);
  if (e == hipSuccess) e = hipMalloc(&v64, na * 8);
  if (e == hipSuccess) e = hipMalloc(&k64, na * 8);
  if (e == hipSuccess) e = hipMalloc(&s64, na * 8);
  if (e == hipSuccess) e = hipMalloc(&idx_sc, na * 8);
  if (e == hipSuccess) e = hipMalloc(&kb_sc, na * 8);
  if (e == hipSuccess) e = hipMalloc(&vb_sc, na * 8);
  if (e == hipSuccess && dd_keys) e = hipMalloc(&dref, na * 8);
  if (e == hipSuccess) e = hipMalloc(&d_maxrow, 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemsetAsync(err, 0, 4, s);
  hipMemsetAsync(d_maxrow, 0, 8, s);
  uint32_t grid = (uint32_t)(((n + THREADS - 1) / THREADS) < 8192
                                 ? ((n + THREADS - 1) / THREADS) : 8192);
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(k_mvcc_flags, dim3(grid), dim3(THREADS), 0, s,
                     d_keys, d_ko, d_vals, d_vo, n, read_ts,
                     dd_keys, dd_ko, dd_vo, dn, dref, vis, ksz, vsz, err);
  hipLaunchKernelGGL(k_mvcc_widen, dim3(grid), dim3(THREADS), 0, s,
                     vis, ksz, vsz, n, v64, k64, s64);
  unsigned int h_err = 0;
  hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) { freeall(); return -1; }
  if (h_err & 1) { freeall(); return -1; }
  if (h_err & 2) { freeall(); *unsupported = 1; return -3; }
  /* exclusive sums */
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, v64, idx_sc, (int)n, s);
  if (hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, v64, idx_sc, (int)n, s);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, k64, kb_sc, (int)n, s);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, s64, vb_sc, (int)n, s);
  /* totals = last scan + last size */
  uint64_t t_idx = 0, t_kb = 0, t_vb = 0, l_idx = 0, l_kb = 0, l_vb = 0;
  if (n) {
    hipMemcpyAsync(&t_idx, idx_sc + n - 1, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&t_kb, kb_sc + n - 1, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&t_vb, vb_sc + n - 1, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&l_idx, v64 + n - 1, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&l_kb, k64 + n - 1, 8, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(&l_vb, s64 + n - 1, 8, hipMemcpyDeviceToHost, s);
  }
  if (hipStreamSynchronize(s) != hipSuccess) { freeall(); return -1; }
  uint64_t n_vis = t_idx + l_idx, ktot = t_kb + l_kb, vtot = t_vb + l_vb;
  /* outputs (region-owned; +2 KiB slack like copr_region_create) */
  uint8_t *o_keys = nullptr, *o_vals = nullptr;
  uint64_t *o_ko = nullptr, *o_vo = nullptr;
  e = hipMalloc(&o_keys, ktot + 2048);
  if (e == hipSuccess) e = hipMalloc(&o_vals, vtot + 2048);
  if (e == hipSuccess) e = hipMalloc(&o_ko, (n_vis + 1) * 8 + 64);
  if (e == hipSuccess) e = hipMalloc(&o_vo, (n_vis + 1) * 8 + 64);
  if (e != hipSuccess) {
    hipFree(o_keys); hipFree(o_vals); hipFree(o_ko); hipFree(o_vo);
    freeall();
    return -2;
  }
  hipLaunchKernelGGL(k_mvcc_gather, dim3(grid), dim3(THREADS), 0, s,
                     d_keys, d_ko, d_vals, d_vo, n, dd_vals, dd_vo, dref,
                     vis, ksz, vsz,
                     idx_sc, kb_sc, vb_sc, o_keys, o_ko, o_vals, o_vo, d_maxrow);
  hipMemcpyAsync(o_ko + n_vis, &ktot, 8, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(o_vo + n_vis, &vtot, 8, hipMemcpyHostToDevice, s);
  unsigned long long h_maxrow = 0;
  hipMemcpyAsync(&h_maxrow, d_maxrow, 8, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) {
    hipFree(o_keys); hipFree(o_vals); hipFree(o_ko); hipFree(o_vo);
    freeall();
    return -1;
  }
  freeall();
  out->d_keys = o_keys;
  out->d_key_offs = o_ko;
  out->d_vals = o_vals;
  out->d_val_offs = o_vo;
  out->n_kv = n_vis;
  out->key_bytes = ktot;
  out->val_bytes = vtot;
  out->max_row_bytes = (uint32_t)h_maxrow;
  return 0;
}

/* ---------------- device TypeChunk encode (project, fixed-8 columns) ----
 * chunk/column.rs:41-71,1052-1071 wire layout built ON DEVICE for output
 * schemas whose columns all chunk-encode as 8-byte fixed values (ints,
 * DOUBLE, DURATION). The host keeps the batch-ladder chunk segmentation
 * (from the keep flags) and patches the 8-byte [len][null_cnt] headers;
 * kernels decode each kept row's datums straight out of the resident
 * value stream and write the data sections + null bitmaps in place —
 * no span-stream D2H, no serial re-encode. Rows the device cannot encode
 * (v2 DURATION cells, decimal/bytes datums under an int schema, short v2
 * real payloads) raise the err flag and the caller falls back to the
 * host path, which reproduces the reference behaviour exactly. */
__global__ static void __launch_bounds__(THREADS)
k_u8_widen(const uint8_t *__restrict__ f, uint64_t n,
           uint64_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = f[i];
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

__global__ static void __launch_bounds__(THREADS)
k_chunk_decode(const uint8_t *__restrict__ keep,
               const uint64_t *__restrict__ out_pos, uint64_t scan_end,
               uint64_t total_rows,
               const unsigned long long *__restrict__ cells, int n_out,
               const uint8_t *__restrict__ vals,
               const uint64_t *__restrict__ val_offs,
               const long long *__restrict__ filt_vals,
               const uint8_t *__restrict__ filt_state,
               const long long *__restrict__ dec2_vals,
               const uint8_t *__restrict__ dec2_state,
               const long long *__restrict__ handles,
               const ChunkColSpec *__restrict__ specs, int n_cols,
               const uint64_t *__restrict__ chunk_prefix, uint32_t n_chunks,
               long long *__restrict__ tmp_vals,
               uint8_t *__restrict__ tmp_null,
               unsigned int *__restrict__ null_cnt,
               unsigned int *__restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < scan_end; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!keep[i]) continue;
    uint64_t pos = out_pos[i];
    if (pos >= total_rows) continue;             /* beyond LIMIT */
    uint32_t ck = d_chunk_of(chunk_prefix, n_chunks, pos);
    uint64_t rs = val_offs[i];
    bool v2row = (val_offs[i + 1] - rs) > 1 && vals[rs] == 128;
    for (int c = 0; c < n_cols; c++) {
      const ChunkColSpec sp = specs[c];
      long long v = 0;
      uint8_t nul = 0;
      if (sp.kind == 1) {
        v = handles[i];
      } else if (sp.kind == 2 || sp.kind == 3) {
        uint8_t st = sp.kind == 2 ? filt_state[i] : dec2_state[i];
        if (st == 0) v = sp.kind == 2 ? filt_vals[i] : dec2_vals[i];
        else if (st == 1 || sp.missing_null) nul = 1;
        else v = sp.missing_val;
      } else {
        unsigned long long cp = cells[(uint64_t)i * n_out + sp.j];
        uint32_t clen = (uint32_t)(cp & 0xFFFFFu);
        if (clen == 0xFFFFFu) {                  /* missing column */
          if (sp.missing_null) nul = 1;
          else v = sp.missing_val;
        } else if (clen == 0xFFFFEu) {           /* explicit v2 NULL */
          nul = 1;
        } else {
          const uint8_t *p = vals + (cp >> 20);
          if (v2row) {
            /* raw v2 payload (compat_v1.rs:28-126 -> chunk decode) */
            if (sp.is_real == 1) {
              /* DOUBLE: payload is the comparable f64 (flag-5 transform) */
              if (clen != 8) { atomicOr(err, 1u); continue; }
              uint64_t u = 0;
              for (int b = 0; b < 8; b++) u = (u << 8) | p[b];
              if (u & 0x8000000000000000ull) u &= 0x7FFFFFFFFFFFFFFFull;
              else u = ~u;
              v = (long long)u;
            } else if (sp.is_real == 2) {        /* duration etc: host */
              atomicOr(err, 1u); continue;
            } else if (sp.uns) {
              if (clen != 1 && clen != 2 && clen != 4 && clen != 8) {
                atomicOr(err, 1u); continue;
              }
              uint64_t u = 0;
              for (uint32_t b = 0; b < clen; b++)
                u |= (uint64_t)p[b] << (8 * b);
              v = (long long)u;
            } else {
              int64_t iv;
              if (!d_v2_int(p, clen, false, &iv)) { atomicOr(err, 1u); continue; }
              v = iv;
            }
          } else {
            CellView cell;
            d_parse_datum(p, clen, &cell);
            if (!cell.len) { atomicOr(err, 1u); continue; }
            if (cell.is_null) nul = 1;
            else if (cell.has_int || cell.has_real) v = cell.ival;
            else { atomicOr(err, 1u); continue; } /* decimal/bytes: host */
          }
        }
      }
      tmp_vals[(uint64_t)c * total_rows + pos] = v;
      tmp_null[(uint64_t)c * total_rows + pos] = nul;
      if (nul)
        atomicAdd(&null_cnt[(uint64_t)ck * n_cols + c], 1u);
    }
  }
}

__global__ static void __launch_bounds__(THREADS)
k_chunk_fill(uint64_t total_rows, int n_cols,
             const long long *__restrict__ tmp_vals,
             const uint8_t *__restrict__ tmp_null,
             const uint64_t *__restrict__ chunk_prefix, uint32_t n_chunks,
             const uint64_t *__restrict__ data_off,  /* [n_chunks*n_cols] */
             const uint64_t *__restrict__ bmp_off,   /* ~0ull = no bitmap */
             uint8_t *__restrict__ outbuf) {
  for (uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       pos < total_rows; pos += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t ck = d_chunk_of(chunk_prefix, n_chunks, pos);
    uint64_t r = pos - chunk_prefix[ck];
    uint64_t clen = (ck + 1 < n_chunks ? chunk_prefix[ck + 1]
                                       : total_rows) - chunk_prefix[ck];
    for (int c = 0; c < n_cols; c++) {
      uint8_t nul = tmp_null[(uint64_t)c * total_rows + pos];
      uint64_t uv = nul ? 0ull
                        : (uint64_t)tmp_vals[(uint64_t)c * total_rows + pos];
      uint64_t doff = data_off[(uint64_t)ck * n_cols + c] + 8 * r;
      #pragma unroll
      for (int b = 0; b < 8; b++) outbuf[doff + b] = (uint8_t)(uv >> (8 * b));
      /* null bitmap: the (r%8==0) thread composes each byte — exactly one
         writer per byte, plain byte stores, no RMW against the data bytes */
      uint64_t bo = bmp_off[(uint64_t)ck * n_cols + c];
      if (bo != ~0ull && (r & 7) == 0) {
        uint8_t byte = 0;
        for (uint64_t k = 0; k < 8 && r + k < clen; k++)
          if (!tmp_null[(uint64_t)c * total_rows + pos + k])
            byte |= (uint8_t)(1u << k);
        outbuf[bo + (r >> 3)] = byte;
      }
    }
  }
}

int dev_chunk_encode(const ProjectOut &po, const DevRegion &rgn, int idxp,
                     uint64_t scan_end, const ChunkColSpec *h_specs,
                     int n_cols, int n_out,
                     const std::vector<uint64_t> &chunk_rows, void *stream,
                     std::vector<uint8_t> *out_resp) {
  hipStream_t s = (hipStream_t)stream;
  /* index project spans reference the KEY stream; keys start with 't',
     never 128, so the v2-row sniff in k_chunk_decode stays inert */
  const uint8_t *d_span = idxp ? rgn.d_keys : rgn.d_vals;
  const uint64_t *d_span_offs = idxp ? rgn.d_key_offs : rgn.d_val_offs;
  uint32_t n_chunks = (uint32_t)chunk_rows.size();
  std::vector<uint64_t> prefix(n_chunks + 1, 0);
  for (uint32_t k = 0; k < n_chunks; k++)
    prefix[k + 1] = prefix[k] + chunk_rows[k];
  uint64_t total = prefix[n_chunks];
  out_resp->clear();
  if (!total) return 0;
  uint64_t *d_outpos = nullptr, *d_prefix = nullptr;
  uint64_t *d_doff = nullptr, *d_boff = nullptr, *k64 = nullptr;
  long long *d_tmpv = nullptr;
  uint8_t *d_tmpn = nullptr, *d_out = nullptr;
  unsigned int *d_nullcnt = nullptr, *d_err = nullptr;
  ChunkColSpec *d_specs = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(d_outpos); hipFree(d_prefix); hipFree(d_doff); hipFree(d_boff);
    hipFree(k64); hipFree(d_tmpv); hipFree(d_tmpn); hipFree(d_out);
    hipFree(d_nullcnt); hipFree(d_err); hipFree(d_specs); hipFree(tmp);
  };
  hipError_t e = hipSuccess;
  uint64_t na = scan_end ? scan_end : 1;
  uint64_t nm = (uint64_t)n_chunks * n_cols;
  if (e == hipSuccess) e = hipMalloc(&d_outpos, na * 8);
  if (e == hipSuccess) e = hipMalloc(&k64, na * 8);
  if (e == hipSuccess) e = hipMalloc(&d_prefix, (n_chunks + 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_tmpv, (uint64_t)n_cols * total * 8);
  if (e == hipSuccess) e = hipMalloc(&d_tmpn, (uint64_t)n_cols * total);
  if (e == hipSuccess) e = hipMalloc(&d_nullcnt, nm * 4);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMalloc(&d_specs, n_cols * sizeof(ChunkColSpec));
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemcpyAsync(d_prefix, prefix.data(), (n_chunks + 1) * 8,
                 hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_specs, h_specs, n_cols * sizeof(ChunkColSpec),
                 hipMemcpyHostToDevice, s);
  hipMemsetAsync(d_nullcnt, 0, nm * 4, s);
  hipMemsetAsync(d_err, 0, 4, s);
  uint32_t grid = (uint32_t)(((scan_end + THREADS - 1) / THREADS) < 8192
                                 ? ((scan_end + THREADS - 1) / THREADS)
                                 : 8192);
  if (!grid) grid = 1;
  hipLaunchKernelGGL(k_u8_widen, dim3(grid), dim3(THREADS), 0, s,
                     po.keep, scan_end, k64);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, k64, d_outpos,
                                   (int)scan_end, s);
  if (hipMalloc(&tmp, tmpb ? tmpb : 16) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, k64, d_outpos, (int)scan_end, s);
  hipLaunchKernelGGL(k_chunk_decode, dim3(grid), dim3(THREADS), 0, s,
                     po.keep, d_outpos, scan_end, total, po.cells, n_out,
                     d_span, d_span_offs, po.filt_vals, po.filt_state,
                     po.dec2_vals, po.dec2_state, po.handles, d_specs, n_cols,
                     d_prefix, n_chunks, d_tmpv, d_tmpn, d_nullcnt, d_err);
  std::vector<unsigned int> h_nullcnt(nm);
  unsigned int h_err = 0;
  e = hipMemcpyAsync(h_nullcnt.data(), d_nullcnt, nm * 4,
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }
  /* section layout (column.rs flush order): per chunk per col
     [len u32][null_cnt u32][bitmap if null_cnt>0][data 8*len] */
  std::vector<uint64_t> h_doff(nm), h_boff(nm, ~0ull);
  uint64_t off = 0;
  for (uint32_t k = 0; k < n_chunks; k++) {
    uint64_t len = chunk_rows[k];
    for (int c = 0; c < n_cols; c++) {
      off += 8;
      if (h_nullcnt[(uint64_t)k * n_cols + c] > 0) {
        h_boff[(uint64_t)k * n_cols + c] = off;
        off += (len + 7) / 8;
      }
      h_doff[(uint64_t)k * n_cols + c] = off;
      off += 8 * len;
    }
  }
  uint64_t total_bytes = off;
  if (e == hipSuccess) e = hipMalloc(&d_doff, nm * 8);
  if (e == hipSuccess) e = hipMalloc(&d_boff, nm * 8);
  if (e == hipSuccess) e = hipMalloc(&d_out, total_bytes);
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemcpyAsync(d_doff, h_doff.data(), nm * 8, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_boff, h_boff.data(), nm * 8, hipMemcpyHostToDevice, s);
  uint32_t grid2 = (uint32_t)(((total + THREADS - 1) / THREADS) < 8192
                                  ? ((total + THREADS - 1) / THREADS) : 8192);
  if (!grid2) grid2 = 1;
  hipLaunchKernelGGL(k_chunk_fill, dim3(grid2), dim3(THREADS), 0, s,
                     total, n_cols, d_tmpv, d_tmpn, d_prefix, n_chunks,
                     d_doff, d_boff, d_out);
  out_resp->resize(total_bytes);
  e = hipMemcpyAsync(out_resp->data(), d_out, total_bytes,
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) { out_resp->clear(); return -1; }
  /* patch the per-(chunk,col) headers */
  for (uint32_t k = 0; k < n_chunks; k++) {
    uint64_t len = chunk_rows[k];
    for (int c = 0; c < n_cols; c++) {
      uint64_t bmb = h_boff[(uint64_t)k * n_cols + c] != ~0ull
                         ? (len + 7) / 8 : 0;
      uint8_t *hw = out_resp->data() +
                    (h_doff[(uint64_t)k * n_cols + c] - bmb - 8);
      uint32_t nc2 = h_nullcnt[(uint64_t)k * n_cols + c];
      hw[0] = (uint8_t)len;  hw[1] = (uint8_t)(len >> 8);
      hw[2] = (uint8_t)(len >> 16); hw[3] = (uint8_t)(len >> 24);
      hw[4] = (uint8_t)nc2;  hw[5] = (uint8_t)(nc2 >> 8);
      hw[6] = (uint8_t)(nc2 >> 16); hw[7] = (uint8_t)(nc2 >> 24);
    }
  }
  return 0;
}

/* ---------------- launch wrappers ----------------
 * k_scan_agg and k_scan_agg_pipe take the same arguments, so one NAGGS
 * switch picks the instance and one launch serves both. */
template <bool IS_HASH>
static int launch_agg(const ScanPlan &plan, const DevRegion &rgn,
                      SimpleAggAcc *d_simple, HashAggTable ht, hipStream_t s,
                      uint32_t grid) {
  void (*kern)(ScanPlan, const uint8_t *, const uint64_t *, uint64_t,
               SimpleAggAcc *, HashAggTable);
  if (plan.use_pipe && !IS_HASH && !plan.index_mode && plan.n_aggs == 1 &&
      plan.aggs[0].kind == DAGG_COUNT_ROWS && plan.has_filter &&
      !plan.filter2_on && !plan.rpn_on && !plan.filter_is_real) {
    /* one int filter column + count(*): the specialised parse */
    kern = k_scan_agg_pipe<1, false, true>;
  } else {
    #define CASE(N)                                                          \
      kern = plan.use_pipe ? k_scan_agg_pipe<N, IS_HASH>                     \
                           : k_scan_agg<N, IS_HASH>
    switch (plan.n_aggs) {
      case 1: CASE(1); break;
      case 2: CASE(2); break;
      case 3: CASE(3); break;
      case 4: CASE(4); break;
      default: CASE(COPR_MAX_AGGS); break;
    }
    #undef CASE
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), plan.lds_bytes, s, plan,
                     rgn.d_vals, rgn.d_val_offs, rgn.n_kv, d_simple, ht);
  return (int)hipGetLastError();
}


/* ================= extract / stream-agg / TopN =================
 * Shared extract pass: per row write (keep/key-null/key) for the plan's
 * group (or order-by) column plus per-agg contribution values; the
 * stream-agg and TopN pipelines below consume these columnar arrays.
 * StreamAgg: groups are contiguous runs of equal keys in input order
 * (stream_aggr_executor.rs:108-117). TopN: n smallest under the order
 * comparator, NULL first, desc reverses (top_n_executor.rs). */
struct ExtractOut {
  uint8_t *st;       /* 0 filtered out; 1 kept NULL key; 2 kept value key */
  int64_t *gkey;
  int64_t *av;       /* [NAGGS][n] contribution values */
  uint8_t *as_;      /* [NAGGS][n] 1 = contributes */
  /* bytes group keys (SlowHashAggregationImpl, slow_hash_aggr_executor.rs:
     220,285): the group column's DECODED payload span in the region's
     value stream + a 64-bit FNV-1a fingerprint (grouping is verified
     byte-exact downstream, the hash only orders candidates) */
  uint64_t *ghash;
  uint64_t *gofs;
  uint32_t *glen;
};

__device__ static inline uint64_t d_fnv1a(const uint8_t *p, uint32_t n) {
  uint64_t h = 1469598103934665603ull;
  for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

/* payload span of a COMPACT_BYTES datum at cell_off (flag 2 + varint len +
   raw payload; byte.rs:518-530). Returns false for other encodings. */
__device__ static inline bool d_compact_bytes_span(const uint8_t *vp,
                                                   uint32_t vlen,
                                                   uint32_t cell_off,
                                                   uint32_t *pofs,
                                                   uint32_t *plen) {
  if (cell_off >= vlen || vp[cell_off] != 2) return false;
  int64_t n;
  uint32_t nb;
  if (!d_var_i64(vp + cell_off + 1, vlen - cell_off - 1, &n, &nb)) return false;
  if (n < 0 || cell_off + 1 + nb + (uint64_t)n > vlen) return false;
  *pofs = cell_off + 1 + nb;
  *plen = (uint32_t)n;
  return true;
}

template <int NAGGS>
__global__ void __launch_bounds__(256)
k_scan_extract(ScanPlan plan, const uint8_t *__restrict__ vals,
               const uint64_t *__restrict__ val_offs, uint64_t n_rows,
               ExtractOut eo, unsigned int *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t rpt = plan.rows_per_tile;
  const uint64_t n_tiles = (n_rows + rpt - 1) / rpt;
  bool any_err = false;

  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t row0 = tile * rpt;
    uint64_t row1 = min(row0 + rpt, n_rows);
    uint64_t gbase = val_offs[row0];
    uint32_t tlen = (uint32_t)(val_offs[row1] - gbase);
    __syncthreads();
    uint32_t shift = stage_tile(vals, gbase, tlen, lds);

    for (uint64_t my_row = row0 + threadIdx.x; my_row < row1;
         my_row += blockDim.x) {
      const uint8_t *vp = lds + shift + (uint32_t)(val_offs[my_row] - gbase);
      uint32_t vlen = (uint32_t)(val_offs[my_row + 1] - val_offs[my_row]);
      const bool GBYTES = eo.ghash != nullptr;
      uint64_t g_h = 0, g_o = 0; uint32_t g_l = 0;
      RowVals rv{};
      AggColView cols[NAGGS > 0 ? NAGGS : 1] = {};
      const uint8_t *db = plan.celldir;
      const uint64_t dn = plan.celldir_n;
      /* in index mode vp IS the index key (extract_launch streams the key
         slab); a bytes group key is not served there */
      bool parse_ok =
          !(GBYTES && plan.index_mode) &&
          d_row_collect<(NAGGS > 0 ? NAGGS : 1), true, true>(
              plan, vp, vlen, my_row,
              [&](int32_t, int64_t cid) -> uint32_t {
                return (uint32_t)db[(uint64_t)(cid - 1) * dn + my_row];
              },
              rv, cols, GBYTES);
      if (!GBYTES || plan.index_mode) {
      } else if (vlen && vp[0] == 128) {
        V2Row r2;
        if (!parse_ok) {
        } else if (d_v2_parse(vp, vlen, &r2)) {
          uint32_t s2, e2;
          int vst = d_v2_find(r2, plan.group_col_id, &s2, &e2);
          if (vst >= 0) {
            rv.grp_found = true;
            if (vst == 0) rv.grp_null = true;
            else {
              /* v2 cells hold the raw payload already */
              const uint8_t *pp = r2.vals + s2;
              g_h = d_fnv1a(pp, e2 - s2);
              g_o = val_offs[my_row] + (uint32_t)(pp - vp);
              g_l = e2 - s2;
            }
          }
        } else parse_ok = false;
      } else if (rv.grp_found && !rv.grp_null) {
        uint32_t po, plen2;
        if (d_compact_bytes_span(vp, vlen, rv.grp_off, &po, &plen2)) {
          g_h = d_fnv1a(vp + po, plen2);
          g_o = val_offs[my_row] + po;
          g_l = plen2;
        } else parse_ok = false;
      }

      uint8_t s = 0;
      int64_t xv0_ = 0, xv1_ = 0;
      uint8_t xn0_ = 0, xn1_ = 0;
      if (plan.n_xcap)
        d_xcap_extract(plan, cols, &xv0_, &xn0_, &xv1_, &xn1_);
      if (!parse_ok) {
        any_err = true;
      } else if (bool ke = false;
                 d_keep2(plan, rv.filt_found, rv.filt_null, rv.filt_v,
                         rv.f2_found, rv.f2_null, rv.f2_v, &ke, xv0_, xn0_,
                         xv1_, xn1_)
                     ? true
                     : (ke ? (any_err = true, false) : false)) {
        s = (rv.grp_found && !rv.grp_null) ? 2 : 1;
      }
      eo.st[my_row] = s;
      eo.gkey[my_row] = rv.grp_v;
      if (GBYTES) {
        eo.ghash[my_row] = s == 2 ? g_h : 0;
        eo.gofs[my_row] = g_o;
        eo.glen[my_row] = s == 2 ? g_l : 0;
      }
      #pragma unroll
      for (int a = 0; a < NAGGS; a++) {
        if (a >= plan.n_aggs) break;   /* buffers are sized n_aggs */
        const DevAggSpec &sp = plan.aggs[a];
        uint8_t contribute = 0;
        int64_t v = 0;
        if (s) {
          if (sp.kind == DAGG_XCAP) {
            /* capture-only channel: no contribution downstream */
          } else if (sp.kind == DAGG_FIRST) {
            /* first row's value, NULL (or missing->NULL) included */
            contribute = (cols[a].found && !cols[a].null) ? 1 : 2;
            v = cols[a].iv;
          } else if (sp.kind == DAGG_COUNT_ROWS) {
            contribute = 1;
          } else if (!cols[a].found || cols[a].null) {
          } else if (sp.kind == DAGG_COUNT_COL) {
            contribute = 1;
          } else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_REAL ||
                     d_is_fold(sp.kind)) {
            contribute = 1; v = cols[a].iv;
          } else {  /* SUM_DEC */
            int d = sp.target_frac - cols[a].dfr;
            if (!cols[a].has_dec || d < 0 || d > 18) {
              any_err = true;
            } else {
              int64_t scale = 1;
              for (int t = 0; t < d; t++) scale *= 10;
              v = cols[a].dsc * scale;
              contribute = 1;
            }
          }
        }
        eo.as_[(uint64_t)a * n_rows + my_row] = contribute;
        eo.av[(uint64_t)a * n_rows + my_row] = v;
      }
    }
  }
  if (any_err) atomicOr(err, 1u);
}

__global__ static void k_st_keep_flags(const uint8_t *st, uint32_t *f,
                                       uint64_t n, uint8_t want_lo,
                                       uint8_t want_hi) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = (st[i] >= want_lo && st[i] <= want_hi) ? 1u : 0u;
}

/* gather kept rows' key/state (+ per-agg) into compacted arrays */
__global__ static void k_compact_rows(const uint8_t *st, const int64_t *gkey,
                                      const int64_t *av, const uint8_t *as_,
                                      const uint64_t *pos, uint64_t n,
                                      uint64_t m, int n_aggs, int64_t *ck,
                                      uint8_t *cs, int64_t *cav, uint8_t *cas,
                                      uint32_t *crow) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !st[i]) return;
  uint64_t p = pos[i];
  ck[p] = gkey[i];
  cs[p] = st[i];
  if (crow) crow[p] = (uint32_t)i;
  for (int a = 0; a < n_aggs; a++) {
    cav[(uint64_t)a * m + p] = av[(uint64_t)a * n + i];
    cas[(uint64_t)a * m + p] = as_[(uint64_t)a * n + i];
  }
}

__global__ static void k_run_flags(const int64_t *ck, const uint8_t *cs,
                                   uint32_t *f, uint64_t m) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  f[i] = (i == 0 || ck[i] != ck[i - 1] || cs[i] != cs[i - 1]) ? 1u : 0u;
}

/* per-compacted-row aggregate update into the run's accumulator slots */
__global__ static void k_run_update(const int64_t *ck, const uint8_t *cs,
                                    const int64_t *cav, const uint8_t *cas,
                                    const uint32_t *segid, uint64_t m,
                                    ScanPlan plan, SimpleAggAcc *accs,
                                    long long *gk, uint8_t *gs) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t seg = segid[i] - 1;
  if (i == 0 || segid[i] != segid[i - 1]) {
    gk[seg] = ck[i];
    gs[seg] = cs[i];
  }
  SimpleAggAcc *base = accs + (uint64_t)seg * plan.n_aggs;
  for (int a = 0; a < plan.n_aggs; a++) {
    const DevAggSpec &sp = plan.aggs[a];
    uint8_t ct = cas[(uint64_t)a * m + i];
    if (sp.kind == DAGG_FIRST) {
      /* runs are contiguous in input order: the boundary row IS the
         group's first row */
      if (i == 0 || segid[i] != segid[i - 1]) {
        base[a].cnt = 1;
        base[a].sum_lo = (unsigned long long)cav[(uint64_t)a * m + i];
        base[a].sum_hi = ct == 2 ? 1 : 0;
      }
      continue;
    }
    if (!ct) continue;
    int64_t v = cav[(uint64_t)a * m + i];
    atomicAdd(&base[a].cnt, 1ull);
    if (sp.kind == DAGG_SUM_REAL)
      atomicAdd((double *)&base[a].sum_lo, __longlong_as_double(v));
    else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_DEC)
      atomic_add_i128(&base[a].sum_lo, &base[a].sum_hi, v);
    else if (d_is_fold(sp.kind)) {
      unsigned long long b = d_fold_xform(sp.kind, v, sp.col_unsigned);
      if (d_is_xor(sp.kind)) atomicXor(&base[a].sum_lo, b);
      else if (sp.kind == DAGG_MAX_INT || sp.kind == DAGG_MIN_INT || sp.kind == DAGG_MAX_REAL || sp.kind == DAGG_MIN_REAL)
        atomicMax(&base[a].sum_lo, b);
      else atomicOr(&base[a].sum_lo, b);
    }
  }
}

__global__ static void k_sort_keys(const int64_t *ck, const uint8_t *cs,
                                   const uint64_t *pos, const uint32_t *crow,
                                   uint64_t m, int uns, int desc,
                                   unsigned long long *skey, uint32_t *srow) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  unsigned long long k = (unsigned long long)ck[i];
  if (!uns) k ^= 0x8000000000000000ull;
  if (desc) k = ~k;
  skey[i] = k;
  srow[i] = crow[i];
  (void)cs; (void)pos;
}

__global__ static void k_gather_kr(const uint8_t *st, const int64_t *gkey,
                                   const uint64_t *pos, const uint32_t *f,
                                   uint64_t n, int64_t *ck, uint32_t *crow) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !f[i]) return;
  uint64_t p = pos[i];
  ck[p] = gkey[i];
  crow[p] = (uint32_t)i;
}

static int extract_launch(const ScanPlan &plan, const DevRegion &rgn,
                          const ExtractOut &eo, unsigned int *d_err,
                          hipStream_t s) {
  uint64_t n_tiles = (rgn.n_kv + plan.rows_per_tile - 1) / plan.rows_per_tile;
  uint32_t grid = (uint32_t)(n_tiles < 4096 ? n_tiles : 4096);
  if (grid == 0) grid = 1;
  /* index mode streams the KEY slab; the value stream rides the aux
     pointers (unique-index handles) */
  ScanPlan p2 = plan;
  DevRegion r2 = rgn;
  if (plan.index_mode) {
    r2.d_vals = rgn.d_keys;
    r2.d_val_offs = rgn.d_key_offs;
    r2.val_bytes = rgn.key_bytes;
    r2.max_row_bytes = rgn.max_key_bytes;
    p2.aux_vals = rgn.d_vals;
    p2.aux_val_offs = rgn.d_val_offs;
    p2.aux_max_vlen = rgn.max_row_bytes;
  }
  const ScanPlan &plan_ = p2;
  const DevRegion &rgn_ = r2;
  #define XCASE(NA)                                                           \
    case NA:                                                                  \
      hipLaunchKernelGGL((k_scan_extract<NA>), dim3(grid), dim3(256),         \
                         plan_.lds_bytes, s, plan_, rgn_.d_vals,              \
                         rgn_.d_val_offs, rgn_.n_kv, eo, d_err);              \
      break
  switch (plan.n_aggs) {
    XCASE(0); XCASE(1); XCASE(2); XCASE(3); XCASE(4);
    XCASE(5); XCASE(6); XCASE(7);
    default: XCASE(COPR_MAX_AGGS); break;
  }
  #undef XCASE
  return (int)hipGetLastError();
}

/* Stream aggregation: extract -> compact kept rows -> run boundaries ->
 * per-run accumulators. Returns n_runs (>=0) or -1 internal, -2 oom,
 * -3 row parse error. Results are copied into the host vectors in run
 * order. */
int dev_stream_agg(const ScanPlan &plan, const DevRegion &rgn, void *stream,
                   std::vector<SimpleAggAcc> *h_accs,
                   std::vector<long long> *h_gk, std::vector<uint8_t> *h_gs) {
  hipStream_t s = (hipStream_t)stream;
  uint64_t n = rgn.n_kv;
  if (!n) return 0;
  uint8_t *st = nullptr, *as_ = nullptr, *cs = nullptr, *cas = nullptr;
  uint8_t *gs = nullptr;
  int64_t *gkey = nullptr, *av = nullptr, *ck = nullptr, *cav = nullptr;
  long long *gk = nullptr;
  uint32_t *f32 = nullptr, *segid = nullptr;
  uint64_t *pos = nullptr;
  unsigned int *d_err = nullptr;
  SimpleAggAcc *accs = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(st); hipFree(as_); hipFree(cs); hipFree(cas); hipFree(gs);
    hipFree(gkey); hipFree(av); hipFree(ck); hipFree(cav); hipFree(gk);
    hipFree(f32); hipFree(segid); hipFree(pos); hipFree(d_err);
    hipFree(accs); hipFree(tmp);
  };
  int na = plan.n_aggs;
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&st, n);
  if (e == hipSuccess) e = hipMalloc(&gkey, n * 8);
  if (e == hipSuccess) e = hipMalloc(&av, (uint64_t)na * n * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&as_, (uint64_t)na * n + 8);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, s);
  if (e != hipSuccess) { freeall(); return -2; }
  ExtractOut eo{st, gkey, av, as_, nullptr, nullptr, nullptr};
  if (extract_launch(plan, rgn, eo, d_err, s)) { freeall(); return -1; }
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (e == hipSuccess) e = hipMalloc(&f32, n * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&pos, n * 8 + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_st_keep_flags, dim3(blocks), dim3(256), 0, s, st, f32,
                     n, 1, 2);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, f32, pos, (int)n, s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, f32, pos, (int)n, s);
  uint64_t m = 0;
  uint32_t last_f = 0;
  e = hipMemcpyAsync(&m, pos + (n - 1), 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&last_f, f32 + (n - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  m += last_f;
  if (!m) { freeall(); return 0; }

  uint64_t ma = m;
  if (e == hipSuccess) e = hipMalloc(&ck, ma * 8);
  if (e == hipSuccess) e = hipMalloc(&cs, ma);
  if (e == hipSuccess) e = hipMalloc(&cav, (uint64_t)na * ma * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&cas, (uint64_t)na * ma + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_compact_rows, dim3(blocks), dim3(256), 0, s, st, gkey,
                     av, as_, pos, n, m, na, ck, cs, cav, cas,
                     (uint32_t *)nullptr);

  uint32_t mblocks = (uint32_t)((m + 255) / 256);
  if (hipMalloc(&segid, ma * 4) != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_run_flags, dim3(mblocks), dim3(256), 0, s, ck, cs, f32,
                     m);
  size_t tmpb2 = 0;
  hipcub::DeviceScan::InclusiveSum(nullptr, tmpb2, f32, segid, (int)m, s);
  if (tmpb2 > tmpb) {
    hipFree(tmp); tmp = nullptr;
    if (hipMalloc(&tmp, tmpb2) != hipSuccess) { freeall(); return -2; }
    tmpb = tmpb2;
  }
  hipcub::DeviceScan::InclusiveSum(tmp, tmpb2, f32, segid, (int)m, s);
  uint32_t n_seg = 0;
  e = hipMemcpyAsync(&n_seg, segid + (m - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }

  if (e == hipSuccess) e = hipMalloc(&accs, (uint64_t)n_seg * na *
                                                sizeof(SimpleAggAcc));
  if (e == hipSuccess) e = hipMalloc(&gk, (uint64_t)n_seg * 8);
  if (e == hipSuccess) e = hipMalloc(&gs, n_seg);
  if (e == hipSuccess)
    e = hipMemsetAsync(accs, 0, (uint64_t)n_seg * na * sizeof(SimpleAggAcc), s);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_run_update, dim3(mblocks), dim3(256), 0, s, ck, cs,
                     cav, cas, segid, m, plan, accs, gk, gs);
  h_accs->resize((size_t)n_seg * na);
  h_gk->resize(n_seg);
  h_gs->resize(n_seg);
  e = hipMemcpyAsync(h_accs->data(), accs,
                     (uint64_t)n_seg * na * sizeof(SimpleAggAcc),
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_gk->data(), gk, (uint64_t)n_seg * 8,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_gs->data(), gs, n_seg, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) return -1;
  return (int)n_seg;
}

/* TopN winner selection: extract the order column, split kept rows into
 * NULL-key and value-key lists (both in source order), radix-sort the
 * value list (stable -> ties keep arrival order), and take the first n
 * per the NULL-first / desc rules. Returns 0 (winners filled), -1
 * internal, -2 oom, -3 parse error. */
int dev_topn_select(const ScanPlan &plan, const DevRegion &rgn,
                    uint64_t topn_n, int desc, void *stream,
                    std::vector<uint32_t> *winners) {
  hipStream_t s = (hipStream_t)stream;
  uint64_t n = rgn.n_kv;
  winners->clear();
  if (!n || !topn_n) return 0;
  uint8_t *st = nullptr, *cs = nullptr, *cas = nullptr;
  int64_t *gkey = nullptr, *ck = nullptr, *cav = nullptr;
  uint32_t *f32 = nullptr, *crow = nullptr, *srow = nullptr, *srow2 = nullptr;
  uint64_t *pos = nullptr;
  unsigned long long *skey = nullptr, *skey2 = nullptr;
  unsigned int *d_err = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(st); hipFree(cs); hipFree(cas); hipFree(gkey); hipFree(ck);
    hipFree(cav); hipFree(f32); hipFree(crow); hipFree(srow); hipFree(srow2);
    hipFree(pos); hipFree(skey); hipFree(skey2); hipFree(d_err); hipFree(tmp);
  };
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&st, n);
  if (e == hipSuccess) e = hipMalloc(&gkey, n * 8);
  /* no aggregates, but the predicate's capture-only slots sit at
     aggs[0..n_xcap) and the extract pass collects exactly n_aggs columns
     (one at least): with two of them n_aggs = 0 would leave the second
     channel reading as 0. The pass writes one (unused) contribution cell per
     slot and row. */
  const uint64_t nx = plan.n_xcap > 0 ? (uint64_t)plan.n_xcap : 0;
  if (e == hipSuccess) e = hipMalloc(&cav, nx ? nx * n * 8 : 16);
  if (e == hipSuccess) e = hipMalloc(&cas, nx ? nx * n : 16);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, s);
  if (e != hipSuccess) { freeall(); return -2; }
  ExtractOut eo{st, gkey, (int64_t *)cav, cas, nullptr, nullptr, nullptr};
  ScanPlan p0 = plan;
  p0.n_aggs = (int32_t)nx;
  if (extract_launch(p0, rgn, eo, d_err, s)) { freeall(); return -1; }
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (e == hipSuccess) e = hipMalloc(&f32, n * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&pos, n * 8 + 8);
  if (e != hipSuccess) { freeall(); return -2; }

  /* pass A: NULL-key rows (st==1); pass B: value rows (st==2) */
  std::vector<uint32_t> a_rows, b_rows_sorted;
  for (int pass = 0; pass < 2; pass++) {
    uint8_t want = pass == 0 ? 1 : 2;
    hipLaunchKernelGGL(k_st_keep_flags, dim3(blocks), dim3(256), 0, s, st,
                       f32, n, want, want);
    size_t tb = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tb, f32, pos, (int)n, s);
    if (tb > tmpb) {
      hipFree(tmp); tmp = nullptr;
      if (hipMalloc(&tmp, tb) != hipSuccess) { freeall(); return -2; }
      tmpb = tb;
    }
    hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, f32, pos, (int)n, s);
    uint64_t m = 0;
    uint32_t lf = 0;
    e = hipMemcpyAsync(&m, pos + (n - 1), 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(&lf, f32 + (n - 1), 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { freeall(); return -1; }
    m += lf;
    if (!m) continue;
    /* gather (key,row); reuse a tiny "state" compact with want-only rows */
    if (ck) { hipFree(ck); ck = nullptr; }
    if (cs) { hipFree(cs); cs = nullptr; }
    if (crow) { hipFree(crow); crow = nullptr; }
    if (e == hipSuccess) e = hipMalloc(&ck, m * 8);
    if (e == hipSuccess) e = hipMalloc(&cs, m);
    if (e == hipSuccess) e = hipMalloc(&crow, m * 4);
    if (e != hipSuccess) { freeall(); return -2; }
    hipLaunchKernelGGL(k_gather_kr, dim3(blocks), dim3(256), 0, s, st, gkey,
                       pos, f32, n, ck, crow);
    if (pass == 0) {
      a_rows.resize(m);
      e = hipMemcpyAsync(a_rows.data(), crow, m * 4, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) { freeall(); return -1; }
      /* only the first topn_n can matter */
      if (a_rows.size() > topn_n) a_rows.resize(topn_n);
    } else {
      uint32_t mb = (uint32_t)((m + 255) / 256);
      if (e == hipSuccess) e = hipMalloc(&skey, m * 8);
      if (e == hipSuccess) e = hipMalloc(&skey2, m * 8);
      if (e == hipSuccess) e = hipMalloc(&srow, m * 4);
      if (e == hipSuccess) e = hipMalloc(&srow2, m * 4);
      if (e != hipSuccess) { freeall(); return -2; }
      hipLaunchKernelGGL(k_sort_keys, dim3(mb), dim3(256), 0, s, ck, cs, pos,
                         crow, m, plan.group_col_unsigned, desc, skey, srow);
      size_t tb = 0;
      hipcub::DeviceRadixSort::SortPairs(nullptr, tb, skey, skey2, srow,
                                         srow2, (int)m, 0, 64, s);
      if (tb > tmpb) {
        hipFree(tmp); tmp = nullptr;
        if (hipMalloc(&tmp, tb) != hipSuccess) { freeall(); return -2; }
        tmpb = tb;
      }
      hipcub::DeviceRadixSort::SortPairs(tmp, tmpb, skey, skey2, srow, srow2,
                                         (int)m, 0, 64, s);
      uint64_t take = m < topn_n ? m : topn_n;
      b_rows_sorted.resize(take);
      e = hipMemcpyAsync(b_rows_sorted.data(), srow2, take * 4,
                         hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) { freeall(); return -1; }
    }
  }
  freeall();
  /* order: asc -> NULLs first; desc -> NULLs last */
  if (!desc) {
    for (uint32_t r : a_rows) {
      if (winners->size() >= topn_n) break;
      winners->push_back(r);
    }
    for (uint32_t r : b_rows_sorted) {
      if (winners->size() >= topn_n) break;
      winners->push_back(r);
    }
  } else {
    for (uint32_t r : b_rows_sorted) {
      if (winners->size() >= topn_n) break;
      winners->push_back(r);
    }
    for (uint32_t r : a_rows) {
      if (winners->size() >= topn_n) break;
      winners->push_back(r);
    }
  }
  return 0;
}

/* ---- multi-key TopN: the two steps that need this file's row
 * parsers; the pipeline itself is topn_multi.hip ---- */

/* keep decision of the scan path for every row: st[i] != 0 = kept. gkey is
 * [n] scratch for the extract pass's group slot (the plan's group column is
 * order key 0). */
int dev_topn_keep_flags(const ScanPlan &plan, const DevRegion &rgn,
                        uint8_t *st, int64_t *gkey, unsigned int *d_err,
                        void *stream) {
  ExtractOut eo{st, gkey, nullptr, nullptr, nullptr, nullptr, nullptr};
  ScanPlan p0 = plan;
  p0.n_aggs = 0;
  return extract_launch(p0, rgn, eo, d_err, (hipStream_t)stream);
}

/* One order key for cnt rows named by rows[]: locate the cell as the plane
 * builder does (directory byte, or a row walk without one; row-v2 through
 * d_v2_find / d_v2_int with the request's signedness), fill an absent cell
 * from the column default, and write topn_key_encode's (rank, u). */
__global__ void __launch_bounds__(256)
k_topn_keys(const uint8_t *__restrict__ vals,
            const uint64_t *__restrict__ val_offs,
            const uint8_t *__restrict__ dirp,
            const uint32_t *__restrict__ rows, uint64_t cnt, TopnKey key,
            unsigned long long *__restrict__ u_out,
            uint8_t *__restrict__ rank_out, unsigned int *__restrict__ err) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool any_err = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt;
       i += stride) {
    ChanRes cr = d_plane_resolve(dirp, rows[i], key.col_id, key.uns != 0, 0,
                                 vals, val_offs);
    any_err |= (cr.fl & CH_ERR) != 0;
    bool is_null;
    int64_t v;
    if (cr.fl & CH_FOUND) {
      is_null = (cr.fl & CH_NULL) != 0;
      v = cr.v;
    } else {
      is_null = key.missing_null != 0;
      v = key.missing_val;
    }
    uint8_t rk;
    unsigned long long u;
    topn_key_encode(v, is_null, key.uns != 0, key.desc != 0, &rk, &u);
    u_out[i] = u;
    rank_out[i] = rk;
  }
  if (any_err) atomicOr(err, 1u);
}

int dev_topn_keys_launch(const DevRegion &rgn, const uint32_t *d_rows,
                         uint64_t cnt, const TopnKey &key,
                         unsigned long long *d_u, uint8_t *d_rank,
                         unsigned int *d_err, void *stream) {
  if (!cnt) return 0;
  const uint8_t *dirp =
      (rgn.d_celldir && key.col_id >= 1 && key.col_id <= 16)
          ? rgn.d_celldir + (uint64_t)(key.col_id - 1) * rgn.n_kv : nullptr;
  uint32_t grid = (uint32_t)min((cnt + 255) / 256, (uint64_t)16384);
  hipLaunchKernelGGL(k_topn_keys, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, rgn.d_vals, rgn.d_val_offs, dirp,
                     d_rows, cnt, key, d_u, d_rank, d_err);
  return (int)hipGetLastError();
}



/* compact a global hash table's occupied slots (keys + accumulator rows)
 * into dense arrays so the host readback scales with n_groups, not with
 * the table size */
__global__ static void k_fill_keys(long long *keys, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = (long long)0x8000000000000000ll;
}

void dev_fill_keys(long long *keys, uint64_t n, void *stream) {
  uint32_t blocks = (uint32_t)((n + 255) / 256);
  hipLaunchKernelGGL(k_fill_keys, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, keys, n);
}

__global__ static void k_ht_flags(const long long *keys, uint32_t tsize,
                                  uint32_t *f) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < tsize)
    f[i] = keys[i] != (long long)0x8000000000000000ll ? 1u : 0u;
}

__global__ static void k_ht_gather(const long long *keys,
                                   const SimpleAggAcc *accs,
                                   const unsigned long long *ext,
                                   uint32_t tsize,
                                   const uint64_t *pos, int n_aggs,
                                   long long *ck, SimpleAggAcc *caccs,
                                   unsigned long long *cext) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= tsize || keys[i] == (long long)0x8000000000000000ll) return;
  uint64_t p = pos[i];
  ck[p] = keys[i];
  for (int a = 0; a < n_aggs; a++) {
    caccs[p * n_aggs + a] = accs[(uint64_t)i * n_aggs + a];
    if (ext) {
      cext[(p * n_aggs + a) * 2] = ext[((uint64_t)i * n_aggs + a) * 2];
      cext[(p * n_aggs + a) * 2 + 1] = ext[((uint64_t)i * n_aggs + a) * 2 + 1];
    }
  }
}

/* returns n_groups (>=0) with host vectors filled, or -1/-2 */
int dev_ht_compact(const HashAggTable &ht, uint32_t tsize, int n_aggs,
                   void *stream, std::vector<long long> *h_keys,
                   std::vector<SimpleAggAcc> *h_accs,
                   std::vector<unsigned long long> *h_ext) {
  hipStream_t s = (hipStream_t)stream;
  uint32_t *f = nullptr;
  uint64_t *pos = nullptr;
  long long *ck = nullptr;
  SimpleAggAcc *caccs = nullptr;
  unsigned long long *cext = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(f); hipFree(pos); hipFree(ck); hipFree(caccs); hipFree(cext);
    hipFree(tmp);
  };
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&f, (uint64_t)tsize * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&pos, (uint64_t)tsize * 8 + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  uint32_t blocks = (tsize + 255) / 256;
  hipLaunchKernelGGL(k_ht_flags, dim3(blocks), dim3(256), 0, s, ht.keys,
                     tsize, f);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, f, pos, (int)tsize, s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, f, pos, (int)tsize, s);
  uint64_t g = 0;
  uint32_t lf = 0;
  e = hipMemcpyAsync(&g, pos + (tsize - 1), 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&lf, f + (tsize - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  g += lf;
  h_keys->resize(g);
  h_accs->resize(g * n_aggs);
  if (h_ext) h_ext->assign(g * n_aggs * 2, 0ull);
  if (g) {
    if (e == hipSuccess) e = hipMalloc(&ck, g * 8);
    if (e == hipSuccess)
      e = hipMalloc(&caccs, g * n_aggs * sizeof(SimpleAggAcc));
    if (e == hipSuccess && ht.ext && h_ext)
      e = hipMalloc(&cext, g * n_aggs * 16);
    if (e != hipSuccess) { freeall(); return -2; }
    hipLaunchKernelGGL(k_ht_gather, dim3(blocks), dim3(256), 0, s, ht.keys,
                       ht.accs, (h_ext ? ht.ext : nullptr), tsize, pos,
                       n_aggs, ck, caccs, cext);
    e = hipMemcpyAsync(h_keys->data(), ck, g * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h_accs->data(), caccs,
                         g * n_aggs * sizeof(SimpleAggAcc),
                         hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cext)
      e = hipMemcpyAsync(h_ext->data(), cext, g * n_aggs * 16,
                         hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  freeall();
  if (e != hipSuccess) return -1;
  return (int)g;
}

/* ---- bytes-group hash agg pipeline (SlowHashAggregationImpl) ---- */
__global__ static void k_compact_bytes(const uint8_t *st, const uint64_t *gh,
                                       const uint64_t *go, const uint32_t *gl,
                                       const int64_t *av, const uint8_t *as_,
                                       const uint64_t *pos, uint64_t n,
                                       uint64_t m, int n_aggs, uint64_t *ch,
                                       uint64_t *co, uint32_t *cl, uint8_t *cs,
                                       int64_t *cav, uint8_t *cas,
                                       uint32_t *idx) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !st[i]) return;
  uint64_t p = pos[i];
  ch[p] = gh[i];
  co[p] = go[i];
  cl[p] = gl[i];
  cs[p] = st[i];
  idx[p] = (uint32_t)p;
  for (int a = 0; a < n_aggs; a++) {
    cav[(uint64_t)a * m + p] = av[(uint64_t)a * n + i];
    cas[(uint64_t)a * m + p] = as_[(uint64_t)a * n + i];
  }
}

/* boundary flags over the hash-sorted permutation: a new group starts when
 * state/hash differ, or the hash ties but the payload bytes differ
 * (grouping stays byte-exact; the hash only clusters candidates) */
__global__ static void k_bytes_boundary(const uint64_t *ch, const uint64_t *co,
                                        const uint32_t *cl, const uint8_t *cs,
                                        const uint32_t *perm,
                                        const uint8_t *vals, uint64_t m,
                                        int int_keys, uint32_t *f) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (i == 0) { f[0] = 1; return; }
  uint32_t a = perm[i], b = perm[i - 1];
  uint32_t nf = 0;
  if (cs[a] != cs[b]) nf = 1;
  else if (cs[a] == 2) {
    if (ch[a] != ch[b]) nf = 1;
    else if (!int_keys) {
      /* fingerprint tie: verify payload bytes (grouping stays exact) */
      if (cl[a] != cl[b]) nf = 1;
      else {
        const uint8_t *pa = vals + co[a], *pb = vals + co[b];
        for (uint32_t t = 0; t < cl[a]; t++)
          if (pa[t] != pb[t]) { nf = 1; break; }
      }
    }
  }
  f[i] = nf;
}

__global__ static void k_iota32(uint32_t *p, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (uint32_t)i;
}

__global__ static void k_bytes_update(const uint64_t *co, const uint32_t *cl,
                                      const uint8_t *cs, const int64_t *cav,
                                      const uint8_t *cas,
                                      const uint32_t *perm,
                                      const uint32_t *segid, uint64_t m,
                                      ScanPlan plan, SimpleAggAcc *accs,
                                      uint64_t *rofs, uint32_t *rlen,
                                      uint8_t *rst) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t seg = segid[i] - 1;
  uint32_t a0 = perm[i];
  if (i == 0 || segid[i] != segid[i - 1]) {
    rofs[seg] = co[a0];
    rlen[seg] = cl[a0];
    rst[seg] = cs[a0];
  }
  SimpleAggAcc *base = accs + (uint64_t)seg * plan.n_aggs;
  for (int a = 0; a < plan.n_aggs; a++) {
    const DevAggSpec &sp = plan.aggs[a];
    if (sp.kind == DAGG_FIRST) {
      /* min source (compacted) index via max of its complement */
      atomicMax(&base[a].cnt, ~(unsigned long long)a0);
      continue;
    }
    if (!cas[(uint64_t)a * m + a0]) continue;
    int64_t v = cav[(uint64_t)a * m + a0];
    atomicAdd(&base[a].cnt, 1ull);
    if (sp.kind == DAGG_SUM_REAL)
      atomicAdd((double *)&base[a].sum_lo, __longlong_as_double(v));
    else if (sp.kind == DAGG_SUM_INT || sp.kind == DAGG_SUM_DEC)
      atomic_add_i128(&base[a].sum_lo, &base[a].sum_hi, v);
    else if (d_is_fold(sp.kind)) {
      unsigned long long b = d_fold_xform(sp.kind, v, sp.col_unsigned);
      if (d_is_xor(sp.kind)) atomicXor(&base[a].sum_lo, b);
      else if (sp.kind == DAGG_MAX_INT || sp.kind == DAGG_MIN_INT || sp.kind == DAGG_MAX_REAL || sp.kind == DAGG_MIN_REAL)
        atomicMax(&base[a].sum_lo, b);
      else atomicOr(&base[a].sum_lo, b);
    }
  }
}

__global__ static void k_bytes_first_fix(const int64_t *cav,
                                         const uint8_t *cas,
                                         const uint32_t *perm,
                                         const uint32_t *segid, uint64_t m,
                                         ScanPlan plan,
                                         SimpleAggAcc *accs) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t seg = segid[i] - 1;
  uint32_t a0 = perm[i];
  SimpleAggAcc *base = accs + (uint64_t)seg * plan.n_aggs;
  for (int a = 0; a < plan.n_aggs; a++) {
    if (plan.aggs[a].kind != DAGG_FIRST) continue;
    if (base[a].cnt == ~(unsigned long long)a0) {
      base[a].sum_lo = (unsigned long long)cav[(uint64_t)a * m + a0];
      base[a].sum_hi = cas[(uint64_t)a * m + a0] == 2 ? 1 : 0;
    }
  }
}

__global__ static void k_bytes_first_norm(uint64_t n_seg, ScanPlan plan,
                                          SimpleAggAcc *accs) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seg) return;
  SimpleAggAcc *base = accs + i * plan.n_aggs;
  for (int a = 0; a < plan.n_aggs; a++)
    if (plan.aggs[a].kind == DAGG_FIRST) base[a].cnt = 1;
}

/* Bytes-key hash aggregation. Returns n_groups (>=0), -1 internal, -2 oom,
 * -3 parse error. Group keys returned as (ofs,len) spans into the region's
 * value stream + the representative state byte (1 = NULL group). */
int dev_bytes_agg(const ScanPlan &plan, const DevRegion &rgn, void *stream,
                  std::vector<SimpleAggAcc> *h_accs,
                  std::vector<uint64_t> *h_kofs, std::vector<uint32_t> *h_klen,
                  std::vector<uint8_t> *h_kst) {
  hipStream_t s = (hipStream_t)stream;
  uint64_t n = rgn.n_kv;
  if (!n) return 0;
  uint8_t *st = nullptr, *as_ = nullptr, *cs = nullptr, *cas = nullptr;
  uint8_t *rst = nullptr;
  int64_t *gkey = nullptr, *av = nullptr, *cav = nullptr;
  uint64_t *gh = nullptr, *go = nullptr, *ch = nullptr, *co = nullptr;
  uint64_t *ch2 = nullptr, *rofs = nullptr, *pos = nullptr;
  uint32_t *gl = nullptr, *cl = nullptr, *f32 = nullptr, *segid = nullptr;
  uint32_t *idx = nullptr, *perm = nullptr, *rlen = nullptr;
  unsigned int *d_err = nullptr;
  SimpleAggAcc *accs = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(st); hipFree(as_); hipFree(cs); hipFree(cas); hipFree(rst);
    hipFree(gkey); hipFree(av); hipFree(cav);
    hipFree(gh); hipFree(go); hipFree(ch); hipFree(co); hipFree(ch2);
    hipFree(rofs); hipFree(pos); hipFree(gl); hipFree(cl); hipFree(f32);
    hipFree(segid); hipFree(idx); hipFree(perm); hipFree(rlen);
    hipFree(d_err); hipFree(accs); hipFree(tmp);
  };
  int na = plan.n_aggs;
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&st, n);
  if (e == hipSuccess) e = hipMalloc(&gkey, n * 8);
  if (e == hipSuccess) e = hipMalloc(&gh, n * 8);
  if (e == hipSuccess) e = hipMalloc(&go, n * 8);
  if (e == hipSuccess) e = hipMalloc(&gl, n * 4);
  if (e == hipSuccess) e = hipMalloc(&av, (uint64_t)na * n * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&as_, (uint64_t)na * n + 8);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, s);
  if (e != hipSuccess) { freeall(); return -2; }
  ExtractOut eo{st, gkey, av, as_, gh, go, gl};
  if (extract_launch(plan, rgn, eo, d_err, s)) { freeall(); return -1; }
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (e == hipSuccess) e = hipMalloc(&f32, n * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&pos, n * 8 + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_st_keep_flags, dim3(blocks), dim3(256), 0, s, st, f32,
                     n, 1, 2);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, f32, pos, (int)n, s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, f32, pos, (int)n, s);
  uint64_t m = 0;
  uint32_t lf = 0;
  e = hipMemcpyAsync(&m, pos + (n - 1), 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&lf, f32 + (n - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  m += lf;
  if (!m) { freeall(); return 0; }

  if (e == hipSuccess) e = hipMalloc(&ch, m * 8);
  if (e == hipSuccess) e = hipMalloc(&ch2, m * 8);
  if (e == hipSuccess) e = hipMalloc(&co, m * 8);
  if (e == hipSuccess) e = hipMalloc(&cl, m * 4);
  if (e == hipSuccess) e = hipMalloc(&cs, m);
  if (e == hipSuccess) e = hipMalloc(&idx, m * 4);
  if (e == hipSuccess) e = hipMalloc(&perm, m * 4);
  if (e == hipSuccess) e = hipMalloc(&cav, (uint64_t)na * m * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&cas, (uint64_t)na * m + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_compact_bytes, dim3(blocks), dim3(256), 0, s, st, gh,
                     go, gl, av, as_, pos, n, m, na, ch, co, cl, cs, cav, cas,
                     idx);
  size_t tb = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ch, ch2, idx, perm, (int)m,
                                     0, 64, s);
  if (tb > tmpb) {
    hipFree(tmp); tmp = nullptr;
    if (hipMalloc(&tmp, tb) != hipSuccess) { freeall(); return -2; }
    tmpb = tb;
  }
  hipcub::DeviceRadixSort::SortPairs(tmp, tmpb, ch, ch2, idx, perm, (int)m, 0,
                                     64, s);
  uint32_t mblocks = (uint32_t)((m + 255) / 256);
  if (hipMalloc(&segid, m * 4) != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_bytes_boundary, dim3(mblocks), dim3(256), 0, s, ch, co,
                     cl, cs, perm, rgn.d_vals, m, /*int_keys=*/0, f32);
  size_t tb2 = 0;
  hipcub::DeviceScan::InclusiveSum(nullptr, tb2, f32, segid, (int)m, s);
  if (tb2 > tmpb) {
    hipFree(tmp); tmp = nullptr;
    if (hipMalloc(&tmp, tb2) != hipSuccess) { freeall(); return -2; }
    tmpb = tb2;
  }
  hipcub::DeviceScan::InclusiveSum(tmp, tmpb, f32, segid, (int)m, s);
  uint32_t n_seg = 0;
  e = hipMemcpyAsync(&n_seg, segid + (m - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }

  if (e == hipSuccess)
    e = hipMalloc(&accs, (uint64_t)n_seg * na * sizeof(SimpleAggAcc));
  if (e == hipSuccess) e = hipMalloc(&rofs, (uint64_t)n_seg * 8);
  if (e == hipSuccess) e = hipMalloc(&rlen, (uint64_t)n_seg * 4);
  if (e == hipSuccess) e = hipMalloc(&rst, n_seg);
  if (e == hipSuccess)
    e = hipMemsetAsync(accs, 0, (uint64_t)n_seg * na * sizeof(SimpleAggAcc), s);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_bytes_update, dim3(mblocks), dim3(256), 0, s, co, cl,
                     cs, cav, cas, perm, segid, m, plan, accs, rofs, rlen,
                     rst);
  bool has_first = false;
  for (int a = 0; a < na; a++)
    if (plan.aggs[a].kind == DAGG_FIRST) has_first = true;
  if (has_first) {
    hipLaunchKernelGGL(k_bytes_first_fix, dim3(mblocks), dim3(256), 0, s,
                       cav, cas, perm, segid, m, plan, accs);
    uint32_t sblocks = (uint32_t)((n_seg + 255) / 256);
    if (sblocks)
      hipLaunchKernelGGL(k_bytes_first_norm, dim3(sblocks), dim3(256), 0, s,
                         (uint64_t)n_seg, plan, accs);
  }
  h_accs->resize((size_t)n_seg * na);
  h_kofs->resize(n_seg);
  h_klen->resize(n_seg);
  h_kst->resize(n_seg);
  e = hipMemcpyAsync(h_accs->data(), accs,
                     (uint64_t)n_seg * na * sizeof(SimpleAggAcc),
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_kofs->data(), rofs, (uint64_t)n_seg * 8,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_klen->data(), rlen, (uint64_t)n_seg * 4,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_kst->data(), rst, n_seg, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) return -1;
  return (int)n_seg;
}


/* ---------------- SST data-block ingestion ----------------
 * RocksDB BlockBasedTable data-block decode on device: restart intervals
 * are independent (each starts with shared=0), so one LANE decodes one
 * interval sequentially, reconstructing prefix-compressed InternalKeys in
 * a per-lane LDS scratch line and stripping the 8-byte trailer. Two
 * passes: sizes -> prefix sums -> materialize. */
#define BLK_MAX_IKEY 128

struct BlkInterval { uint64_t byte_start, byte_end; };

__device__ static inline bool d_blk_varint32(const uint8_t *p, uint64_t rem,
                                             uint32_t *v, uint32_t *n) {
  uint32_t x = 0;
  uint32_t i = 0;
  int sh = 0;
  while (i < rem && i < 5) {
    uint8_t b = p[i++];
    x |= (uint32_t)(b & 0x7F) << sh;
    sh += 7;
    if (!(b & 0x80)) { *v = x; *n = i; return true; }
  }
  return false;
}

template <bool WRITE>
__global__ void __launch_bounds__(256)
k_blk_parse(const uint8_t *__restrict__ blocks,
            const BlkInterval *__restrict__ ivs, uint64_t n_ivs,
            uint32_t *__restrict__ n_entries,
            uint64_t *__restrict__ key_bytes,
            uint64_t *__restrict__ val_bytes,
            const uint64_t *__restrict__ ent_base,
            const uint64_t *__restrict__ kb_base,
            const uint64_t *__restrict__ vb_base,
            uint8_t *__restrict__ out_keys, uint64_t *__restrict__ out_ko,
            uint8_t *__restrict__ out_vals, uint64_t *__restrict__ out_vo,
            unsigned int *__restrict__ err) {
  extern __shared__ uint8_t lds[];
  uint8_t *mykey = lds + (uint64_t)threadIdx.x * BLK_MAX_IKEY;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t iv = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       iv < n_ivs; iv += stride) {
    uint64_t pos = ivs[iv].byte_start;
    const uint64_t end = ivs[iv].byte_end;
    uint32_t klen = 0;
    uint32_t ents = 0;
    uint64_t kb = 0, vb = 0;
    uint64_t ko = WRITE ? kb_base[iv] : 0;
    uint64_t vo = WRITE ? vb_base[iv] : 0;
    uint64_t eb = WRITE ? ent_base[iv] : 0;
    bool bad = false;
    while (pos < end) {
      uint32_t shared, non_shared, vlen, n;
      if (!d_blk_varint32(blocks + pos, end - pos, &shared, &n)) { bad = true; break; }
      pos += n;
      if (!d_blk_varint32(blocks + pos, end - pos, &non_shared, &n)) { bad = true; break; }
      pos += n;
      if (!d_blk_varint32(blocks + pos, end - pos, &vlen, &n)) { bad = true; break; }
      pos += n;
      if (pos + non_shared + vlen > end || shared > klen ||
          shared + non_shared > BLK_MAX_IKEY) { bad = true; break; }
      for (uint32_t t = 0; t < non_shared; t++)
        mykey[shared + t] = blocks[pos + t];
      klen = shared + non_shared;
      pos += non_shared;
      if (klen < 8) { bad = true; break; }
      if (WRITE) {
        out_ko[eb + ents] = ko;
        out_vo[eb + ents] = vo;
        for (uint32_t t = 0; t < klen - 8; t++) out_keys[ko + t] = mykey[t];
        ko += klen - 8;
        for (uint32_t t = 0; t < vlen; t++) out_vals[vo + t] = blocks[pos + t];
        vo += vlen;
      }
      kb += klen - 8;
      vb += vlen;
      ents++;
      pos += vlen;
    }
    if (bad || pos != end) {
      atomicOr(err, 1u);
      if (!WRITE) { n_entries[iv] = 0; key_bytes[iv] = 0; val_bytes[iv] = 0; }
      continue;
    }
    if (!WRITE) {
      n_entries[iv] = ents;
      key_bytes[iv] = kb;
      val_bytes[iv] = vb;
    }
  }
}

__global__ static void k_blk_widen(const uint32_t *src, uint64_t *dst,
                                   uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

/* parse uncompressed data blocks into a DevRegion. Returns 0, -1 internal,
 * -2 oom, -3 malformed block. h_blocks/h_offs are the HOST copies (restart
 * arrays are read on host to build the interval table). */
int dev_blocks_build(const uint8_t *h_blocks, const uint64_t *h_block_offs,
                     uint32_t n_blocks, DevRegion *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  *out = DevRegion{};
  std::vector<BlkInterval> ivs;
  for (uint32_t b = 0; b < n_blocks; b++) {
    const uint8_t *blk = h_blocks + h_block_offs[b];
    uint64_t blen = h_block_offs[b + 1] - h_block_offs[b];
    if (blen < 8) return -3;
    uint32_t nr = (uint32_t)blk[blen - 4] | ((uint32_t)blk[blen - 3] << 8) |
                  ((uint32_t)blk[blen - 2] << 16) |
                  ((uint32_t)blk[blen - 1] << 24);
    if (blen < 4 + (uint64_t)nr * 4 || nr == 0) return -3;
    uint64_t data_end = blen - 4 - (uint64_t)nr * 4;
    const uint8_t *ra = blk + data_end;
    uint64_t prev = UINT64_MAX;
    for (uint32_t r = 0; r < nr; r++) {
      uint32_t off = (uint32_t)ra[4 * r] | ((uint32_t)ra[4 * r + 1] << 8) |
                     ((uint32_t)ra[4 * r + 2] << 16) |
                     ((uint32_t)ra[4 * r + 3] << 24);
      if (off >= data_end && !(off == 0 && data_end == 0)) return -3;
      if (prev != UINT64_MAX) {
        if (off <= prev) return -3;
        ivs.push_back({h_block_offs[b] + prev, h_block_offs[b] + off});
      }
      prev = off;
    }
    ivs.push_back({h_block_offs[b] + prev, h_block_offs[b] + data_end});
  }
  uint64_t n_ivs = ivs.size();
  uint64_t total = h_block_offs[n_blocks];
  uint8_t *d_blocks = nullptr;
  BlkInterval *d_ivs = nullptr;
  uint32_t *d_ne = nullptr;
  uint64_t *d_kb = nullptr, *d_vb = nullptr;
  uint64_t *d_eb = nullptr, *d_kbb = nullptr, *d_vbb = nullptr;
  uint64_t *d_ne64 = nullptr;
  unsigned int *d_err = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  hipError_t e = hipSuccess;
  auto fail = [&](int rc) {
    hipFree(d_blocks); hipFree(d_ivs); hipFree(d_ne); hipFree(d_kb);
    hipFree(d_vb); hipFree(d_eb); hipFree(d_kbb); hipFree(d_vbb);
    hipFree(d_ne64); hipFree(d_err); hipFree(tmp);
    hipFree(out->d_keys); hipFree(out->d_key_offs);
    hipFree(out->d_vals); hipFree(out->d_val_offs);
    *out = DevRegion{};
    return rc;
  };
  if (e == hipSuccess) e = hipMalloc(&d_blocks, total + 2048);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_blocks, h_blocks, total, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMalloc(&d_ivs, n_ivs * sizeof(BlkInterval) + 16);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_ivs, ivs.data(), n_ivs * sizeof(BlkInterval),
                       hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMalloc(&d_ne, n_ivs * 4 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_ne64, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_kb, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_vb, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_eb, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_kbb, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_vbb, (n_ivs + 1) * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, s);
  if (e != hipSuccess) return fail(-2);
  uint32_t blocks_g = (uint32_t)((n_ivs + 255) / 256);
  if (!blocks_g) blocks_g = 1;
  uint32_t lds_b = 256 * BLK_MAX_IKEY;
  hipLaunchKernelGGL((k_blk_parse<false>), dim3(blocks_g), dim3(256), lds_b,
                     s, d_blocks, d_ivs, n_ivs, d_ne, d_kb, d_vb, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     d_err);
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(-1);
  if (h_err) return fail(-3);
  /* widen entry counts, then exclusive-scan entries/key-bytes/val-bytes */
  hipLaunchKernelGGL(k_blk_widen, dim3(blocks_g), dim3(256), 0, s, d_ne,
                     d_ne64, n_ivs);
  hipMemsetAsync(d_ne64 + n_ivs, 0, 8, s);
  hipMemsetAsync(d_kb + n_ivs, 0, 8, s);
  hipMemsetAsync(d_vb + n_ivs, 0, 8, s);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, d_ne64, d_eb,
                                   (int)(n_ivs + 1), s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) return fail(-2);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, d_ne64, d_eb, (int)(n_ivs + 1),
                                   s);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, d_kb, d_kbb, (int)(n_ivs + 1),
                                   s);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, d_vb, d_vbb, (int)(n_ivs + 1),
                                   s);
  uint64_t n_kv = 0, key_total = 0, val_total = 0;
  e = hipMemcpyAsync(&n_kv, d_eb + n_ivs, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&key_total, d_kbb + n_ivs, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&val_total, d_vbb + n_ivs, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(-1);
  out->n_kv = n_kv;
  out->key_bytes = key_total;
  out->val_bytes = val_total;
  if (e == hipSuccess) e = hipMalloc(&out->d_keys, key_total + 2048);
  if (e == hipSuccess) e = hipMalloc(&out->d_vals, val_total + 2048);
  if (e == hipSuccess) e = hipMalloc(&out->d_key_offs, (n_kv + 1) * 8 + 2048);
  if (e == hipSuccess) e = hipMalloc(&out->d_val_offs, (n_kv + 1) * 8 + 2048);
  if (e != hipSuccess) return fail(-2);
  hipLaunchKernelGGL((k_blk_parse<true>), dim3(blocks_g), dim3(256), lds_b,
                     s, d_blocks, d_ivs, n_ivs, d_ne, d_kb, d_vb, d_eb,
                     d_kbb, d_vbb, out->d_keys, out->d_key_offs, out->d_vals,
                     out->d_val_offs, d_err);
  hipError_t c1 = hipMemcpyAsync(out->d_key_offs + n_kv, &key_total, 8,
                                 hipMemcpyHostToDevice, s);
  hipError_t c2 = hipMemcpyAsync(out->d_val_offs + n_kv, &val_total, 8,
                                 hipMemcpyHostToDevice, s);
  e = hipStreamSynchronize(s);
  hipFree(d_blocks); hipFree(d_ivs); hipFree(d_ne); hipFree(d_kb);
  hipFree(d_vb); hipFree(d_eb); hipFree(d_kbb); hipFree(d_vbb);
  hipFree(d_ne64); hipFree(d_err); hipFree(tmp);
  if (e != hipSuccess || c1 != hipSuccess || c2 != hipSuccess) {
    hipFree(out->d_keys); hipFree(out->d_key_offs);
    hipFree(out->d_vals); hipFree(out->d_val_offs);
    *out = DevRegion{};
    return -1;
  }
  return 0;
}


/* int-key grouped aggregation through the SORTED pipeline: exact u64 key
 * compare (no fingerprint verify). Used when a FastHash request carries
 * FIRST, which the atomic-table path cannot order. Returns like
 * dev_stream_agg; group keys come back in h_gk. */
/* multi-key grouping: the group id stands in for the key the
   extract pass parsed; a kept row always has one */
__global__ static void k_gid_keys(const int64_t *__restrict__ gid,
                                  int64_t *__restrict__ gkey,
                                  uint8_t *__restrict__ st, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  gkey[i] = gid[i];
  st[i] = st[i] ? 2 : 0;
}

int dev_int_sorted_agg(const ScanPlan &plan, const DevRegion &rgn,
                       void *stream, std::vector<SimpleAggAcc> *h_accs,
                       std::vector<long long> *h_gk,
                       std::vector<uint8_t> *h_gs, const int64_t *d_gid) {
  hipStream_t s = (hipStream_t)stream;
  uint64_t n = rgn.n_kv;
  if (!n) return 0;
  uint8_t *st = nullptr, *as_ = nullptr, *cs = nullptr, *cas = nullptr;
  uint8_t *rst = nullptr;
  int64_t *gkey = nullptr, *av = nullptr, *ck = nullptr, *cav = nullptr;
  uint64_t *rofs = nullptr, *pos = nullptr, *ch2 = nullptr;
  uint32_t *cl0 = nullptr, *f32 = nullptr, *segid = nullptr;
  uint32_t *idx = nullptr, *perm = nullptr, *rlen = nullptr;
  unsigned int *d_err = nullptr;
  SimpleAggAcc *accs = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  auto freeall = [&]() {
    hipFree(st); hipFree(as_); hipFree(cs); hipFree(cas); hipFree(rst);
    hipFree(gkey); hipFree(av); hipFree(ck); hipFree(cav); hipFree(rofs);
    hipFree(pos); hipFree(ch2); hipFree(cl0); hipFree(f32); hipFree(segid);
    hipFree(idx); hipFree(perm); hipFree(rlen); hipFree(d_err);
    hipFree(accs); hipFree(tmp);
  };
  int na = plan.n_aggs;
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = hipMalloc(&st, n);
  if (e == hipSuccess) e = hipMalloc(&gkey, n * 8);
  if (e == hipSuccess) e = hipMalloc(&av, (uint64_t)na * n * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&as_, (uint64_t)na * n + 8);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, s);
  if (e != hipSuccess) { freeall(); return -2; }
  ExtractOut eo{st, gkey, av, as_, nullptr, nullptr, nullptr};
  if (extract_launch(plan, rgn, eo, d_err, s)) { freeall(); return -1; }
  if (d_gid)
    hipLaunchKernelGGL(k_gid_keys, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, d_gid, gkey, st, n);
  unsigned int h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  uint32_t blocks = (uint32_t)((n + 255) / 256);
  if (e == hipSuccess) e = hipMalloc(&f32, n * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&pos, n * 8 + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_st_keep_flags, dim3(blocks), dim3(256), 0, s, st, f32,
                     n, 1, 2);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, f32, pos, (int)n, s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, f32, pos, (int)n, s);
  uint64_t m = 0;
  uint32_t lf = 0;
  e = hipMemcpyAsync(&m, pos + (n - 1), 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&lf, f32 + (n - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  m += lf;
  if (!m) { freeall(); return 0; }

  if (e == hipSuccess) e = hipMalloc(&ck, m * 8);
  if (e == hipSuccess) e = hipMalloc(&ch2, m * 8);
  if (e == hipSuccess) e = hipMalloc(&cs, m);
  if (e == hipSuccess) e = hipMalloc(&cl0, m * 4);
  if (e == hipSuccess) e = hipMalloc(&idx, m * 4);
  if (e == hipSuccess) e = hipMalloc(&perm, m * 4);
  if (e == hipSuccess) e = hipMalloc(&cav, (uint64_t)na * m * 8 + 8);
  if (e == hipSuccess) e = hipMalloc(&cas, (uint64_t)na * m + 8);
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemsetAsync(cl0, 0, m * 4, s);
  hipLaunchKernelGGL(k_compact_rows, dim3(blocks), dim3(256), 0, s, st, gkey,
                     av, as_, pos, n, m, na, ck, cs, cav, cas,
                     (uint32_t *)nullptr);
  uint32_t mblocks = (uint32_t)((m + 255) / 256);
  hipLaunchKernelGGL(k_iota32, dim3(mblocks), dim3(256), 0, s, idx, m);
  size_t tb = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t *)ck, ch2,
                                     idx, perm, (int)m, 0, 64, s);
  if (tb > tmpb) {
    hipFree(tmp); tmp = nullptr;
    if (hipMalloc(&tmp, tb) != hipSuccess) { freeall(); return -2; }
    tmpb = tb;
  }
  hipcub::DeviceRadixSort::SortPairs(tmp, tmpb, (const uint64_t *)ck, ch2,
                                     idx, perm, (int)m, 0, 64, s);
  if (hipMalloc(&segid, m * 4) != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_bytes_boundary, dim3(mblocks), dim3(256), 0, s,
                     (const uint64_t *)ck, (const uint64_t *)ck, cl0, cs,
                     perm, rgn.d_vals, m, /*int_keys=*/1, f32);
  size_t tb2 = 0;
  hipcub::DeviceScan::InclusiveSum(nullptr, tb2, f32, segid, (int)m, s);
  if (tb2 > tmpb) {
    hipFree(tmp); tmp = nullptr;
    if (hipMalloc(&tmp, tb2) != hipSuccess) { freeall(); return -2; }
    tmpb = tb2;
  }
  hipcub::DeviceScan::InclusiveSum(tmp, tmpb, f32, segid, (int)m, s);
  uint32_t n_seg = 0;
  e = hipMemcpyAsync(&n_seg, segid + (m - 1), 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }

  if (e == hipSuccess)
    e = hipMalloc(&accs, (uint64_t)n_seg * na * sizeof(SimpleAggAcc));
  if (e == hipSuccess) e = hipMalloc(&rofs, (uint64_t)n_seg * 8);
  if (e == hipSuccess) e = hipMalloc(&rlen, (uint64_t)n_seg * 4);
  if (e == hipSuccess) e = hipMalloc(&rst, n_seg);
  if (e == hipSuccess)
    e = hipMemsetAsync(accs, 0, (uint64_t)n_seg * na * sizeof(SimpleAggAcc), s);
  if (e != hipSuccess) { freeall(); return -2; }
  hipLaunchKernelGGL(k_bytes_update, dim3(mblocks), dim3(256), 0, s,
                     (const uint64_t *)ck, cl0, cs, cav, cas, perm, segid, m,
                     plan, accs, rofs, rlen, rst);
  bool has_first = false;
  for (int a = 0; a < na; a++)
    if (plan.aggs[a].kind == DAGG_FIRST) has_first = true;
  if (has_first) {
    hipLaunchKernelGGL(k_bytes_first_fix, dim3(mblocks), dim3(256), 0, s,
                       cav, cas, perm, segid, m, plan, accs);
    uint32_t sblocks = (uint32_t)((n_seg + 255) / 256);
    if (sblocks)
      hipLaunchKernelGGL(k_bytes_first_norm, dim3(sblocks), dim3(256), 0, s,
                         (uint64_t)n_seg, plan, accs);
  }
  h_accs->resize((size_t)n_seg * na);
  h_gk->resize(n_seg);
  h_gs->resize(n_seg);
  e = hipMemcpyAsync(h_accs->data(), accs,
                     (uint64_t)n_seg * na * sizeof(SimpleAggAcc),
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_gk->data(), rofs, (uint64_t)n_seg * 8,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_gs->data(), rst, n_seg, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) return -1;
  return (int)n_seg;
}

/* gather the given rows (in order) of a region into a new DevRegion */
__global__ static void k_sub_sizes(const uint64_t *ko, const uint64_t *vo,
                                   const uint32_t *rows, uint64_t m,
                                   uint64_t *klen, uint64_t *vlen) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t r = rows[i];
  klen[i] = ko[r + 1] - ko[r];
  vlen[i] = vo[r + 1] - vo[r];
}

__global__ static void k_sub_copy(const uint8_t *src_k, const uint64_t *src_ko,
                                  const uint8_t *src_v, const uint64_t *src_vo,
                                  const uint32_t *rows, uint64_t m,
                                  const uint64_t *dst_ko,
                                  const uint64_t *dst_vo, uint8_t *dst_k,
                                  uint8_t *dst_v) {
  uint64_t i = blockIdx.x;               /* one block per row */
  if (i >= m) return;
  uint32_t r = rows[i];
  uint64_t ks = src_ko[r], kl = src_ko[r + 1] - ks, kd = dst_ko[i];
  for (uint64_t b = threadIdx.x; b < kl; b += blockDim.x)
    dst_k[kd + b] = src_k[ks + b];
  uint64_t vs = src_vo[r], vl = src_vo[r + 1] - vs, vd = dst_vo[i];
  for (uint64_t b = threadIdx.x; b < vl; b += blockDim.x)
    dst_v[vd + b] = src_v[vs + b];
}

int dev_subregion_build(const DevRegion &src, const uint32_t *h_rows,
                        uint64_t m, DevRegion *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  *out = DevRegion{};
  out->n_kv = m;
  uint32_t *d_rows = nullptr;
  uint64_t *klen = nullptr, *vlen = nullptr;
  void *tmp = nullptr;
  size_t tmpb = 0;
  hipError_t e = hipSuccess;
  auto fail = [&](int rc) {
    hipFree(d_rows); hipFree(klen); hipFree(vlen); hipFree(tmp);
    hipFree(out->d_keys); hipFree(out->d_key_offs);
    hipFree(out->d_vals); hipFree(out->d_val_offs);
    *out = DevRegion{};
    return rc;
  };
  if (!m) {
    if (hipMalloc(&out->d_key_offs, 8 + 2048) != hipSuccess) return -2;
    if (hipMalloc(&out->d_val_offs, 8 + 2048) != hipSuccess) return fail(-2);
    if (hipMalloc(&out->d_keys, 2048) != hipSuccess) return fail(-2);
    if (hipMalloc(&out->d_vals, 2048) != hipSuccess) return fail(-2);
    hipMemsetAsync(out->d_key_offs, 0, 8, s);
    hipMemsetAsync(out->d_val_offs, 0, 8, s);
    hipStreamSynchronize(s);
    return 0;
  }
  if (e == hipSuccess) e = hipMalloc(&d_rows, m * 4);
  if (e == hipSuccess) e = hipMalloc(&klen, (m + 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&vlen, (m + 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&out->d_key_offs, (m + 1) * 8 + 2048);
  if (e == hipSuccess) e = hipMalloc(&out->d_val_offs, (m + 1) * 8 + 2048);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_rows, h_rows, m * 4, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return fail(-2);
  uint32_t blocks = (uint32_t)((m + 255) / 256);
  hipLaunchKernelGGL(k_sub_sizes, dim3(blocks), dim3(256), 0, s,
                     src.d_key_offs, src.d_val_offs, d_rows, m, klen, vlen);
  hipMemsetAsync(klen + m, 0, 8, s);
  hipMemsetAsync(vlen + m, 0, 8, s);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, klen, out->d_key_offs,
                                   (int)(m + 1), s);
  if (hipMalloc(&tmp, tmpb) != hipSuccess) return fail(-2);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, klen, out->d_key_offs,
                                   (int)(m + 1), s);
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, vlen, out->d_val_offs,
                                   (int)(m + 1), s);
  uint64_t kb = 0, vb = 0;
  e = hipMemcpyAsync(&kb, out->d_key_offs + m, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&vb, out->d_val_offs + m, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(-1);
  out->key_bytes = kb;
  out->val_bytes = vb;
  if (e == hipSuccess) e = hipMalloc(&out->d_keys, kb + 2048);
  if (e == hipSuccess) e = hipMalloc(&out->d_vals, vb + 2048);
  if (e != hipSuccess) return fail(-2);
  hipLaunchKernelGGL(k_sub_copy, dim3((uint32_t)m), dim3(64), 0, s, src.d_keys,
                     src.d_key_offs, src.d_vals, src.d_val_offs, d_rows, m,
                     out->d_key_offs, out->d_val_offs, out->d_keys,
                     out->d_vals);
  e = hipStreamSynchronize(s);
  hipFree(d_rows); hipFree(klen); hipFree(vlen); hipFree(tmp);
  if (e != hipSuccess) {
    hipFree(out->d_keys); hipFree(out->d_key_offs);
    hipFree(out->d_vals); hipFree(out->d_val_offs);
    *out = DevRegion{};
    return -1;
  }
  return 0;
}

int dev_scan_launch(const ScanPlan &plan, const DevRegion &rgn,
                    SimpleAggAcc *d_simple, const HashAggTable *ht,
                    const ProjectOut *po, void *stream) {
  uint64_t n_tiles = (rgn.n_kv + plan.rows_per_tile - 1) / plan.rows_per_tile;
  uint32_t grid = (uint32_t)(n_tiles < 4096 ? n_tiles : 4096);
  if (grid == 0) grid = 1;
  hipStream_t s = (hipStream_t)stream;
  DevRegion r2 = rgn;
  ScanPlan p2 = plan;
  if (plan.index_mode) {
    /* index scans parse the KEY stream: swap it into the streamed slot;
       the original VALUE stream rides along for unique-index handles and
       new-format layouts (d_index_value_split) */
    r2.d_vals = rgn.d_keys;
    r2.d_val_offs = rgn.d_key_offs;
    r2.val_bytes = rgn.key_bytes;
    r2.max_row_bytes = rgn.max_key_bytes;
    p2.aux_vals = rgn.d_vals;
    p2.aux_val_offs = rgn.d_val_offs;
    p2.aux_max_vlen = rgn.max_row_bytes;
  }
  if (plan.mode == 1)
    return launch_agg<false>(p2, r2, d_simple, HashAggTable{}, s, grid);
  if (plan.mode == 2)
    return launch_agg<true>(p2, r2, nullptr, *ht, s, grid);
  /* project: index mode streams the KEY slab (r2 swap) and reads values
     only through the aux pointers (value handles) */
  hipLaunchKernelGGL(k_scan_project, dim3(grid), dim3(THREADS), plan.lds_bytes,
                     s, p2, r2.d_vals, r2.d_val_offs, rgn.d_keys,
                     rgn.d_key_offs, rgn.n_kv, *po);
  return (int)hipGetLastError();
}

int dev_crc64_launch(const DevRegion &rgn, const uint64_t *d_tables,
                     unsigned long long *d_xor, void *stream) {
  uint64_t n_blk = (rgn.n_kv + THREADS - 1) / THREADS;
  uint32_t grid = (uint32_t)(n_blk < 8192 ? n_blk : 8192);
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(k_crc64_reg, dim3(grid), dim3(THREADS), 0,
                     (hipStream_t)stream, rgn.d_vals, rgn.d_val_offs,
                     rgn.d_keys, rgn.d_key_offs, rgn.n_kv, d_tables, d_xor);
  return (int)hipGetLastError();
}

}  // namespace copr
