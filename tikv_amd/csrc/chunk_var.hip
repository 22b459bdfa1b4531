/* chunk_var.hip — device TypeChunk encode for project responses whose output
 * columns include variable-length bytes and decimals. The
 * fixed-8-only encoder (dev_chunk_encode) stays in kernels.hip.
 *
 * Wire layout per chunk and column (chunk/column.rs:41-71,1052-1071):
 *   [len u32][null_cnt u32][bitmap iff null_cnt > 0]
 *   fixed-8: 8 bytes per row       decimal: 40 bytes per row (zeros = NULL)
 *   bytes:   i64 offsets x (len+1), then the payload bytes back to back
 *
 * Three steps: k_cv_measure places every kept row and records where each
 * cell's bytes are; one exclusive sum per bytes column turns the lengths
 * into payload offsets; k_cv_fill writes the per-row sections and
 * k_cv_payload moves the payload bytes through LDS tiles. */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "copr_internal.h"
#include "datum_dev.h"

namespace copr {

#define CV_THREADS 256u
/* rows of one (chunk, column) that a payload block takes at a time */
#define CV_ITEM_ROWS 256u
/* a payload longer than this is gathered by the whole block, not 8 lanes */
#define CV_LONG_ROW 256u
/* sources are byte offsets into the span stream; this bit marks an offset
   into the per-request defaults buffer instead */
#define CV_SRC_DEFAULT (1ull << 63)
/* k_cv_payload's LDS: the tile (+16 for the destination's misalignment) and
   CV_ITEM_ROWS x 16 B of row descriptors, kept 512 B under 20 KiB (the
   compiler pads the arrays): eight blocks per CU */
static_assert(COPR_CHUNK_TILE_BYTES + 16 + CV_ITEM_ROWS * 16 <= 20480 - 512,
              "payload tile sized for 8 blocks per CU");

/* ---------------- decimal: the chunk form of one binary decimal ----------
 * Device restatement of prod::pdec_decode (read_decimal,
 * decimal.rs:2204-2289) with the host's bounds, so both accept and reject
 * the same payloads. p = [prec][frac][binary decimal]. */

/* encoded length, 0 = rejected (short, prec < frac, more than 9 words) */
__device__ static inline uint32_t d_pdec_need(const uint8_t *p, uint32_t rem) {
  if (rem < 3) return 0;
  uint32_t prec = p[0], fr = p[1];
  if (prec < fr) return 0;
  uint32_t int_cnt = prec - fr;
  uint32_t iw = int_cnt / 9, ld = int_cnt - iw * 9;
  uint32_t fw = fr / 9, td = fr - fw * 9;
  if (iw + (ld ? 1u : 0u) + fw + (td ? 1u : 0u) > 9) return 0;
  uint32_t need = 2 + iw * 4 + DIG2B[ld] + fw * 4 + DIG2B[td];
  return rem < need ? 0 : need;
}

/* p passed d_pdec_need. hdr = int_cnt, frac_cnt, result_frac, negative;
   w = word_buf. false = a word out of range. */
__device__ static inline bool d_pdec_words(const uint8_t *p, uint8_t hdr[4],
                                           uint32_t w[9]) {
  uint32_t prec = p[0], fr = p[1];
  uint32_t int_cnt = prec - fr;
  uint32_t iw = int_cnt / 9, ld = int_cnt - iw * 9;
  uint32_t fw = fr / 9, td = fr - fw * 9;
  const uint8_t *q = p + 2;
  uint32_t mask = (q[0] & 0x80) ? 0u : 0xFFFFFFFFu;
  bool first = true;
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
    return r ^ mask;
  };
  #pragma unroll
  for (int k = 0; k < 9; k++) w[k] = 0;
  uint32_t wi = 0;
  if (ld) {
    uint32_t v = rd_word(DIG2B[ld]);
    if (v >= TEN_POW_D[ld + 1]) return false;      /* the host's bound */
    w[wi] = v;
    if (v) wi++;
    else int_cnt -= ld;                            /* leading zero word */
  }
  for (uint32_t k = 0; k < iw; k++) {
    uint32_t v = rd_word(4);
    if (v > 999999999u) return false;
    w[wi] = v;
    if (wi > 0 || v) wi++;
    else int_cnt -= 9;
  }
  for (uint32_t k = 0; k < fw; k++) {
    uint32_t v = rd_word(4);
    if (v > 999999999u) return false;
    w[wi++] = v;
  }
  if (td) {
    /* trailing digits scale up to a full word */
    uint64_t v = (uint64_t)rd_word(DIG2B[td]) * TEN_POW_D[9 - td];
    if (v > 999999999ull) return false;
    w[wi] = (uint32_t)v;
  }
  hdr[0] = (uint8_t)int_cnt; hdr[1] = (uint8_t)fr; hdr[2] = (uint8_t)fr;
  hdr[3] = mask ? 1 : 0;
  if (int_cnt == 0 && fr == 0) {                   /* Decimal::zero() */
    #pragma unroll
    for (int k = 0; k < 9; k++) w[k] = 0;
    hdr[0] = 1; hdr[3] = 0;
  }
  return true;
}

/* ---------------- 1. measure ---------------------------------------------
 * One lane per scanned row. At the row's output position, per column: the
 * null byte and, in val, the fixed-8 value or the source offset of the
 * payload (bytes) / of [prec] (decimal); bytes columns also record the
 * payload length for the offsets scan. The fixed-8 sourcing restates
 * k_chunk_decode's. */
struct CvSrc {
  const uint8_t *keep;
  const unsigned long long *cells;
  const uint8_t *span;             /* value stream, or key stream (index) */
  const uint64_t *span_offs;
  const long long *filt_vals, *dec2_vals, *handles;
  const uint8_t *filt_state, *dec2_state;
  int32_t n_out;
};

__device__ static inline bool d_cv_fixed8(const ChunkColSpec &sp,
                                          const CvSrc &s, uint64_t i,
                                          bool v2row, long long *out,
                                          uint8_t *nul) {
  long long v = 0;
  *nul = 0;
  if (sp.kind == 1) {
    v = s.handles[i];
  } else if (sp.kind == 2 || sp.kind == 3) {
    uint8_t st = sp.kind == 2 ? s.filt_state[i] : s.dec2_state[i];
    if (st == 0) v = sp.kind == 2 ? s.filt_vals[i] : s.dec2_vals[i];
    else if (st == 1 || sp.missing_null) *nul = 1;
    else v = sp.missing_val;
  } else {
    unsigned long long cp = s.cells[i * s.n_out + sp.j];
    uint32_t clen = (uint32_t)(cp & 0xFFFFFu);
    if (clen == 0xFFFFFu) {                        /* missing column */
      if (sp.missing_null) *nul = 1;
      else v = sp.missing_val;
    } else if (clen == 0xFFFFEu) {                 /* explicit v2 NULL */
      *nul = 1;
    } else {
      const uint8_t *p = s.span + (cp >> 20);
      if (v2row) {
        if (sp.is_real == 1) {
          if (clen != 8) return false;
          uint64_t u = d_be_u64(p);
          if (u & 0x8000000000000000ull) u &= 0x7FFFFFFFFFFFFFFFull;
          else u = ~u;
          v = (long long)u;
        } else if (sp.is_real == 2) {              /* duration: host */
          return false;
        } else {
          int64_t iv;
          if (!d_v2_int(p, clen, sp.uns != 0, &iv)) return false;
          v = iv;
        }
      } else {
        CellView cell;
        d_parse_datum(p, clen, &cell);
        if (!cell.len) return false;
        if (cell.is_null) *nul = 1;
        else if (cell.has_int || cell.has_real) v = cell.ival;
        else return false;
      }
    }
  }
  *out = v;
  return true;
}

__global__ static void __launch_bounds__(CV_THREADS)
k_cv_measure(CvSrc s, const uint64_t *__restrict__ out_pos, uint64_t scan_end,
             uint64_t total, const ChunkVarSpec *__restrict__ specs,
             int n_cols, const uint64_t *__restrict__ chunk_prefix,
             uint32_t n_chunks, unsigned long long *__restrict__ val,
             uint8_t *__restrict__ nulb, uint64_t *__restrict__ lens,
             unsigned int *__restrict__ null_cnt,
             unsigned int *__restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < scan_end; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!s.keep[i]) continue;
    uint64_t pos = out_pos[i];
    if (pos >= total) continue;                    /* beyond LIMIT */
    uint32_t ck = d_chunk_of(chunk_prefix, n_chunks, pos);
    uint64_t rs = s.span_offs[i];
    bool v2row = (s.span_offs[i + 1] - rs) > 1 && s.span[rs] == 128;
    for (int c = 0; c < n_cols; c++) {
      const ChunkVarSpec sp = specs[c];
      unsigned long long v = 0;
      uint64_t blen = 0;
      uint8_t nul = 0;
      if (sp.ctype == 0) {
        long long fv;
        if (!d_cv_fixed8(sp.fx, s, i, v2row, &fv, &nul)) {
          atomicOr(err, 1u);
          continue;
        }
        v = (unsigned long long)fv;
      } else {
        unsigned long long cp = s.cells[i * s.n_out + sp.fx.j];
        uint32_t clen = (uint32_t)(cp & 0xFFFFFu);
        uint64_t off = cp >> 20;
        const uint8_t *p = s.span + off;
        if (clen == 0xFFFFFu) {                    /* missing column */
          if (sp.fx.missing_null) nul = 1;
          else { v = CV_SRC_DEFAULT | sp.def_off; blen = sp.def_len; }
        } else if (clen == 0xFFFFEu) {             /* explicit v2 NULL */
          nul = 1;
        } else if (!v2row && clen == 0) {          /* no v1 datum is empty */
          atomicOr(err, 1u);
          continue;
        } else if (!v2row && clen == 1 && p[0] == 0) {
          nul = 1;                                 /* v1 NIL datum */
        } else if (sp.ctype == 1) {
          if (v2row) {                             /* the raw cell span */
            v = off; blen = clen;
          } else {
            /* flag 2: zigzag varint length, then the bytes. Anything else
               (flag-1 memcomparable bytes, a datum of another type): host */
            int64_t l; uint32_t n;
            if (p[0] != 2 || !d_var_i64(p + 1, clen - 1, &l, &n) || l < 0 ||
                1 + (uint64_t)n + (uint64_t)l != clen) {
              atomicOr(err, 1u);
              continue;
            }
            v = off + 1 + n; blen = (uint64_t)l;
          }
        } else {
          /* [prec][frac][binary decimal], after the flag byte in a v1 cell;
             the cell must end where the decimal ends */
          uint32_t skip = v2row ? 0u : 1u;
          uint32_t need = d_pdec_need(p + skip, clen - skip);
          if ((!v2row && p[0] != 6) || !need || need != clen - skip) {
            atomicOr(err, 1u);
            continue;
          }
          v = off + skip;
        }
      }
      val[(uint64_t)c * total + pos] = v;
      nulb[(uint64_t)c * total + pos] = nul;
      if (sp.ctype == 1) lens[(uint64_t)sp.vidx * (total + 1) + pos] = blen;
      if (nul) atomicAdd(&null_cnt[(uint64_t)ck * n_cols + c], 1u);
    }
  }
}

/* ---------------- 2. offsets ---------------------------------------------
 * pref = exclusive sum of lens over total + 1 entries (the last length is
 * 0), per bytes column. The payload bytes of chunk k are the difference of
 * the prefix at its two boundaries. */
__global__ static void __launch_bounds__(CV_THREADS)
k_cv_totals(const uint64_t *__restrict__ pref, uint64_t total, int n_var,
            const uint64_t *__restrict__ chunk_prefix, uint32_t n_chunks,
            uint64_t *__restrict__ vbytes) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)n_chunks * n_var) return;
  uint32_t k = (uint32_t)(t / n_var);
  uint32_t vi = (uint32_t)(t % n_var);
  const uint64_t *P = pref + (uint64_t)vi * (total + 1);
  vbytes[t] = P[chunk_prefix[k + 1]] - P[chunk_prefix[k]];
}

struct KeepToU64 {
  __host__ __device__ uint64_t operator()(const uint8_t &k) const { return k; }
};

/* ---------------- 3. fill: everything but the payload bytes --------------
 * One lane per output row: bitmaps (the r % 8 == 0 lane composes each byte,
 * one writer per byte), fixed-8 values, decimal structs, bytes offsets. The
 * sections start at arbitrary byte offsets, hence byte stores. */
__device__ static inline void d_put_le(uint8_t *o, uint64_t v, int n) {
  for (int b = 0; b < n; b++) o[b] = (uint8_t)(v >> (8 * b));
}

__global__ static void __launch_bounds__(CV_THREADS)
k_cv_fill(uint64_t total, int n_cols, const ChunkVarSpec *__restrict__ specs,
          const unsigned long long *__restrict__ val,
          const uint8_t *__restrict__ nulb, const uint64_t *__restrict__ pref,
          const uint64_t *__restrict__ chunk_prefix, uint32_t n_chunks,
          const uint64_t *__restrict__ data_off,   /* [n_chunks * n_cols] */
          const uint64_t *__restrict__ bmp_off,    /* ~0ull = no bitmap */
          const uint8_t *__restrict__ span,
          const uint8_t *__restrict__ defaults, uint8_t *__restrict__ outbuf,
          unsigned int *__restrict__ err) {
  for (uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       pos < total; pos += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t ck = d_chunk_of(chunk_prefix, n_chunks, pos);
    uint64_t first = chunk_prefix[ck];
    uint64_t r = pos - first;
    uint64_t clen = chunk_prefix[ck + 1] - first;
    for (int c = 0; c < n_cols; c++) {
      const ChunkVarSpec sp = specs[c];
      const uint8_t *nc = nulb + (uint64_t)c * total;
      uint8_t nul = nc[pos];
      unsigned long long v = val[(uint64_t)c * total + pos];
      uint8_t *d = outbuf + data_off[(uint64_t)ck * n_cols + c];
      if (sp.ctype == 0) {
        d_put_le(d + 8 * r, nul ? 0ull : v, 8);
      } else if (sp.ctype == 1) {
        const uint64_t *P = pref + (uint64_t)sp.vidx * (total + 1);
        uint64_t base = P[first];
        d_put_le(d + 8 * r, P[pos] - base, 8);
        if (r + 1 == clen) d_put_le(d + 8 * clen, P[pos + 1] - base, 8);
      } else {
        uint8_t *o = d + 40 * r;
        if (nul) {
          for (int b = 0; b < 40; b++) o[b] = 0;
        } else if (v & CV_SRC_DEFAULT) {
          const uint8_t *q = defaults + (v & ~CV_SRC_DEFAULT);
          for (int b = 0; b < 40; b++) o[b] = q[b];
        } else {
          uint8_t hdr[4];
          uint32_t w[9];
          if (!d_pdec_words(span + v, hdr, w)) {
            atomicOr(err, 1u);
          } else {
            o[0] = hdr[0]; o[1] = hdr[1]; o[2] = hdr[2]; o[3] = hdr[3];
            #pragma unroll
            for (int k = 0; k < 9; k++) d_put_le(o + 4 + 4 * k, w[k], 4);
          }
        }
      }
      uint64_t bo = bmp_off[(uint64_t)ck * n_cols + c];
      if (bo != ~0ull && (r & 7) == 0) {
        uint8_t byte = 0;
        for (uint64_t k = 0; k < 8 && r + k < clen; k++)
          if (!nc[pos + k]) byte |= (uint8_t)(1u << k);
        outbuf[bo + (r >> 3)] = byte;
      }
    }
  }
}

/* ---------------- 3b. payload bytes --------------------------------------
 * A block takes an item: up to CV_ITEM_ROWS consecutive output rows of one
 * (chunk, bytes column), whose destination bytes are contiguous. It cuts the
 * item into runs that fit the tile. Per run, lanes gather the scattered
 * payloads into LDS at the byte where they land relative to the run's first
 * destination byte (shifted by that byte's misalignment, so that 16-byte
 * LDS words line up with 16-byte words of the response), and the block
 * streams the tile out with aligned 16-byte stores and byte stores at the two
 * ragged ends. A payload that alone exceeds the tile is copied straight from
 * source to destination, each wave moving 1 KiB segments. */
struct CvItem {
  uint64_t pos0;        /* first output row */
  uint32_t n_rows;      /* <= CV_ITEM_ROWS */
  uint32_t chunk;
};

__device__ static inline uint4 d_ld16(const uint8_t *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);                     /* any alignment */
  return v;
}

/* [s, s+len) -> [d, d+len), whole block; 16-byte stores on d's alignment */
__device__ static inline void d_cv_copy_direct(uint8_t *d, const uint8_t *s,
                                               uint64_t len) {
  uint64_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > len) head = len;
  if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
  uint64_t n16 = (len - head) >> 4;
  uint4 *d16 = (uint4 *)(d + head);
  for (uint64_t q = threadIdx.x; q < n16; q += CV_THREADS)
    d16[q] = d_ld16(s + head + 16 * q);
  for (uint64_t j = head + 16 * n16 + threadIdx.x; j < len; j += CV_THREADS)
    d[j] = s[j];
}

__global__ static void __launch_bounds__(CV_THREADS)
k_cv_payload(const CvItem *__restrict__ items, uint32_t n_items,
             const int32_t *__restrict__ varcols, int n_cols, uint64_t total,
             const unsigned long long *__restrict__ val,
             const uint64_t *__restrict__ pref,
             const uint64_t *__restrict__ chunk_prefix,
             const uint64_t *__restrict__ pay_off,  /* [n_chunks * n_cols] */
             const uint8_t *__restrict__ span,
             const uint8_t *__restrict__ defaults,
             uint8_t *__restrict__ outbuf) {
  __shared__ uint4 tile16[(COPR_CHUNK_TILE_BYTES + 16) / 16];
  __shared__ const uint8_t *s_src[CV_ITEM_ROWS];
  __shared__ uint32_t s_off[CV_ITEM_ROWS], s_len[CV_ITEM_ROWS];
  uint8_t *tile = (uint8_t *)tile16;
  const uint32_t tid = threadIdx.x;
  const uint32_t vi = blockIdx.y;
  const int c = varcols[vi];
  const uint64_t *P = pref + (uint64_t)vi * (total + 1);
  const unsigned long long *V = val + (uint64_t)c * total;
  auto source = [&](unsigned long long v) -> const uint8_t * {
    return (v & CV_SRC_DEFAULT) ? defaults + (v & ~CV_SRC_DEFAULT) : span + v;
  };
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const CvItem item = items[it];
    const uint64_t p1 = item.pos0 + item.n_rows;
    /* + P[row] = the row's first byte in the response (mod 2^64) */
    const uint64_t dbase = pay_off[(uint64_t)item.chunk * n_cols + c] -
                           P[chunk_prefix[item.chunk]];
    uint64_t a = item.pos0;
    while (a < p1) {                                  /* a is block-uniform */
      const uint64_t pa = P[a];
      const uint64_t row = a + tid;
      const bool in = row < p1;
      const uint64_t lo = in ? P[row] - pa : 0;
      const uint64_t hi = in ? P[row + 1] - pa : 0;
      /* prefixes only grow: the rows that fit are a leading run. The barrier
         also ends the previous run's reads of the tile. */
      const uint32_t cnt =
          (uint32_t)__syncthreads_count(in && hi <= COPR_CHUNK_TILE_BYTES);
      if (cnt == 0) {                                 /* one oversized row */
        d_cv_copy_direct(outbuf + (dbase + pa), source(V[a]), P[a + 1] - pa);
        a += 1;
        continue;
      }
      const uint64_t nbytes = P[a + cnt] - pa;
      uint8_t *D = outbuf + (dbase + pa);
      const uint32_t shift = (uint32_t)((uintptr_t)D & 15u);
      if (tid < cnt) {
        s_src[tid] = source(V[row]);
        s_off[tid] = shift + (uint32_t)lo;
        s_len[tid] = (uint32_t)(hi - lo);
      }
      __syncthreads();
      /* gather: 8 lanes per row, 32 rows in flight */
      int any_long = 0;
      for (uint32_t r = tid >> 3; r < cnt; r += CV_THREADS / 8) {
        const uint32_t len = s_len[r];
        if (len > CV_LONG_ROW) { any_long = 1; continue; }
        const uint8_t *sp = s_src[r];
        uint8_t *tp = tile + s_off[r];
        for (uint32_t j = tid & 7u; j < len; j += 8) tp[j] = sp[j];
      }
      if (__syncthreads_or(any_long)) {
        /* long rows: the whole block per row, coalesced */
        for (uint32_t r = 0; r < cnt; r++) {
          const uint32_t len = s_len[r];
          if (len <= CV_LONG_ROW) continue;
          const uint8_t *sp = s_src[r];
          uint8_t *tp = tile + s_off[r];
          for (uint32_t j = tid; j < len; j += CV_THREADS) tp[j] = sp[j];
        }
        __syncthreads();
      }
      /* stream out: D + j <- tile[shift + j] */
      uint32_t head = (16u - shift) & 15u;
      if (head > nbytes) head = (uint32_t)nbytes;
      if (tid < head) D[tid] = tile[shift + tid];
      const uint32_t n16 = (uint32_t)((nbytes - head) >> 4);
      uint4 *D16 = (uint4 *)(D + head);
      const uint4 *T16 = tile16 + ((shift + head) >> 4);
      for (uint32_t q = tid; q < n16; q += CV_THREADS) D16[q] = T16[q];
      for (uint32_t j = head + 16 * n16 + tid; j < nbytes; j += CV_THREADS)
        D[j] = tile[shift + j];
      a += cnt;
    }
    __syncthreads();               /* the next item's run reuses the tile */
  }
}

/* ---------------- host: prepare and launch -------------------------------- */
int dev_chunk_encode_var(const ProjectOut &po, const DevRegion &rgn, int idxp,
                         uint64_t scan_end, const ChunkVarSpec *h_specs_in,
                         int n_cols, int n_out, const uint8_t *defaults,
                         size_t def_bytes,
                         const std::vector<uint64_t> &chunk_rows, void *stream,
                         std::vector<uint8_t> *out_resp) {
  hipStream_t s = (hipStream_t)stream;
  uint32_t n_chunks = (uint32_t)chunk_rows.size();
  std::vector<uint64_t> prefix(n_chunks + 1, 0);
  for (uint32_t k = 0; k < n_chunks; k++)
    prefix[k + 1] = prefix[k] + chunk_rows[k];
  const uint64_t total = prefix[n_chunks];
  out_resp->clear();
  if (!total) return 0;
  /* bytes columns get consecutive indices into lens / pref */
  std::vector<ChunkVarSpec> specs(h_specs_in, h_specs_in + n_cols);
  std::vector<int32_t> varcols;
  for (int c = 0; c < n_cols; c++) {
    specs[c].vidx = -1;
    if (specs[c].ctype == 1) {
      specs[c].vidx = (int32_t)varcols.size();
      varcols.push_back(c);
    }
  }
  const int n_var = (int)varcols.size();
  const uint64_t nm = (uint64_t)n_chunks * n_cols;
  const uint64_t nv = (uint64_t)n_chunks * n_var;
  const uint64_t plen = (uint64_t)n_var * (total + 1);

  uint64_t *d_outpos = nullptr, *d_prefix = nullptr, *d_lens = nullptr;
  uint64_t *d_pref = nullptr, *d_vbytes = nullptr, *d_offs = nullptr;
  unsigned long long *d_val = nullptr;
  uint8_t *d_nul = nullptr, *d_out = nullptr, *d_def = nullptr;
  unsigned int *d_nullcnt = nullptr, *d_err = nullptr;
  ChunkVarSpec *d_specs = nullptr;
  int32_t *d_varcols = nullptr;
  CvItem *d_items = nullptr;
  void *tmp = nullptr;
  auto freeall = [&]() {
    hipFree(d_outpos); hipFree(d_prefix); hipFree(d_lens); hipFree(d_pref);
    hipFree(d_vbytes); hipFree(d_offs); hipFree(d_val); hipFree(d_nul);
    hipFree(d_out); hipFree(d_def); hipFree(d_nullcnt); hipFree(d_err);
    hipFree(d_specs); hipFree(d_varcols); hipFree(d_items); hipFree(tmp);
  };
  hipError_t e = hipMalloc(&d_outpos, (scan_end ? scan_end : 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_prefix, (n_chunks + 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_val, (uint64_t)n_cols * total * 8);
  if (e == hipSuccess) e = hipMalloc(&d_nul, (uint64_t)n_cols * total);
  if (e == hipSuccess) e = hipMalloc(&d_lens, (plen ? plen : 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_pref, (plen ? plen : 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_vbytes, (nv ? nv : 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&d_nullcnt, nm * 4);
  if (e == hipSuccess) e = hipMalloc(&d_err, 4);
  if (e == hipSuccess) e = hipMalloc(&d_specs, n_cols * sizeof(ChunkVarSpec));
  if (e == hipSuccess) e = hipMalloc(&d_varcols, (n_var ? n_var : 1) * 4);
  if (e == hipSuccess) e = hipMalloc(&d_def, def_bytes ? def_bytes : 1);
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemcpyAsync(d_prefix, prefix.data(), (n_chunks + 1) * 8,
                 hipMemcpyHostToDevice, s);
  hipMemcpyAsync(d_specs, specs.data(), n_cols * sizeof(ChunkVarSpec),
                 hipMemcpyHostToDevice, s);
  if (n_var)
    hipMemcpyAsync(d_varcols, varcols.data(), n_var * 4, hipMemcpyHostToDevice,
                   s);
  if (def_bytes)
    hipMemcpyAsync(d_def, defaults, def_bytes, hipMemcpyHostToDevice, s);
  hipMemsetAsync(d_nullcnt, 0, nm * 4, s);
  hipMemsetAsync(d_err, 0, 4, s);
  /* lens[total] of every bytes column stays 0 */
  if (plen) hipMemsetAsync(d_lens, 0, plen * 8, s);

  /* output position of every scanned row: exclusive sum of the keep flags */
  hipcub::TransformInputIterator<uint64_t, KeepToU64, const uint8_t *> keep64(
      po.keep, KeepToU64());
  size_t tmpb = 0, tmpb2 = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb, keep64, d_outpos,
                                   (int)scan_end, s);
  if (n_var)
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmpb2, d_lens, d_pref,
                                     (int)(total + 1), s);
  if (tmpb2 > tmpb) tmpb = tmpb2;
  if (hipMalloc(&tmp, tmpb ? tmpb : 16) != hipSuccess) { freeall(); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, keep64, d_outpos, (int)scan_end,
                                   s);
  auto grid_for = [](uint64_t n) {
    uint64_t g = (n + CV_THREADS - 1) / CV_THREADS;
    return (uint32_t)(g < 1 ? 1 : (g < 8192 ? g : 8192));
  };
  CvSrc src;
  src.keep = po.keep;
  src.cells = po.cells;
  /* index project spans reference the KEY stream; keys start with 't',
     never 128, so the v2-row sniff stays inert */
  src.span = idxp ? rgn.d_keys : rgn.d_vals;
  src.span_offs = idxp ? rgn.d_key_offs : rgn.d_val_offs;
  src.filt_vals = po.filt_vals; src.filt_state = po.filt_state;
  src.dec2_vals = po.dec2_vals; src.dec2_state = po.dec2_state;
  src.handles = po.handles;
  src.n_out = n_out;
  hipLaunchKernelGGL(k_cv_measure, dim3(grid_for(scan_end)), dim3(CV_THREADS),
                     0, s, src, d_outpos, scan_end, total, d_specs, n_cols,
                     d_prefix, n_chunks, d_val, d_nul, d_lens, d_nullcnt,
                     d_err);
  for (int vi = 0; vi < n_var; vi++)
    hipcub::DeviceScan::ExclusiveSum(tmp, tmpb, d_lens + vi * (total + 1),
                                     d_pref + vi * (total + 1),
                                     (int)(total + 1), s);
  if (n_var)
    hipLaunchKernelGGL(k_cv_totals, dim3(grid_for(nv)), dim3(CV_THREADS), 0, s,
                       d_pref, total, n_var, d_prefix, n_chunks, d_vbytes);
  /* back to the host: n_chunks x n_cols numbers, no per-row data */
  std::vector<unsigned int> h_nullcnt(nm);
  std::vector<uint64_t> h_vbytes(nv);
  unsigned int h_err = 0;
  e = hipMemcpyAsync(h_nullcnt.data(), d_nullcnt, nm * 4,
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && nv)
    e = hipMemcpyAsync(h_vbytes.data(), d_vbytes, nv * 8,
                       hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { freeall(); return -1; }
  if (h_err) { freeall(); return -3; }

  /* section layout in EChunkCol::flush's order. offs = three arrays of nm:
     data (fixed values / decimal structs / bytes offsets), bitmap, payload */
  std::vector<uint64_t> h_offs(3 * nm, ~0ull);
  uint64_t *h_doff = h_offs.data(), *h_boff = h_doff + nm, *h_poff = h_boff + nm;
  std::vector<CvItem> items;
  uint64_t off = 0;
  for (uint32_t k = 0; k < n_chunks; k++) {
    const uint64_t len = chunk_rows[k];
    for (int c = 0; c < n_cols; c++) {
      const uint64_t m = (uint64_t)k * n_cols + c;
      off += 8;
      if (h_nullcnt[m] > 0) { h_boff[m] = off; off += (len + 7) / 8; }
      h_doff[m] = off;
      if (specs[c].ctype == 0) off += 8 * len;
      else if (specs[c].ctype == 2) off += 40 * len;
      else {
        off += 8 * (len + 1);
        h_poff[m] = off;
        off += h_vbytes[(uint64_t)k * n_var + specs[c].vidx];
      }
    }
    if (n_var)
      for (uint64_t r = 0; r < len; r += CV_ITEM_ROWS) {
        CvItem it;
        it.pos0 = prefix[k] + r;
        it.n_rows = (uint32_t)(len - r < CV_ITEM_ROWS ? len - r : CV_ITEM_ROWS);
        it.chunk = k;
        items.push_back(it);
      }
  }
  const uint64_t total_bytes = off;
  e = hipMalloc(&d_offs, 3 * nm * 8);
  if (e == hipSuccess) e = hipMalloc(&d_out, total_bytes);
  if (e == hipSuccess && n_var)
    e = hipMalloc(&d_items, items.size() * sizeof(CvItem));
  if (e != hipSuccess) { freeall(); return -2; }
  hipMemcpyAsync(d_offs, h_offs.data(), 3 * nm * 8, hipMemcpyHostToDevice, s);
  hipLaunchKernelGGL(k_cv_fill, dim3(grid_for(total)), dim3(CV_THREADS), 0, s,
                     total, n_cols, d_specs, d_val, d_nul, d_pref, d_prefix,
                     n_chunks, d_offs, d_offs + nm, src.span, d_def, d_out,
                     d_err);
  if (n_var) {
    hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(CvItem),
                   hipMemcpyHostToDevice, s);
    uint32_t gx = (uint32_t)(items.size() < 65536 ? items.size() : 65536);
    hipLaunchKernelGGL(k_cv_payload, dim3(gx, (uint32_t)n_var),
                       dim3(CV_THREADS), 0, s, d_items,
                       (uint32_t)items.size(), d_varcols, n_cols, total, d_val,
                       d_pref, d_prefix, d_offs + 2 * nm, src.span, d_def,
                       d_out);
  }
  out_resp->resize(total_bytes);
  e = hipMemcpyAsync(out_resp->data(), d_out, total_bytes,
                     hipMemcpyDeviceToHost, s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  freeall();
  if (e != hipSuccess) { out_resp->clear(); return -1; }
  if (h_err) { out_resp->clear(); return -3; }   /* a decimal word out of range */
  /* patch the per-(chunk,col) headers */
  for (uint32_t k = 0; k < n_chunks; k++) {
    const uint32_t len = (uint32_t)chunk_rows[k];
    for (int c = 0; c < n_cols; c++) {
      const uint64_t m = (uint64_t)k * n_cols + c;
      uint64_t bmb = h_boff[m] != ~0ull ? ((uint64_t)len + 7) / 8 : 0;
      uint8_t *hw = out_resp->data() + (h_doff[m] - bmb - 8);
      const uint32_t nc = h_nullcnt[m];
      for (int b = 0; b < 4; b++) {
        hw[b] = (uint8_t)(len >> (8 * b));
        hw[4 + b] = (uint8_t)(nc >> (8 * b));
      }
    }
  }
  return 0;
}

}  // namespace copr
