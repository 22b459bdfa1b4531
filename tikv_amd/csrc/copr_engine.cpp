/* copr_engine.cpp — PRODUCT C-ABI engine (include/copr_gpu.h).
 *
 * Host side of the MI355X coprocessor batch-executor: descriptor planning
 * (mirrors build_executors, runner.rs:307), region residency, kernel
 * dispatch, and datum response encode (runner.rs:1188 TypeDefault arm via
 * vector.rs:362 / datum_codec.rs:248-294 for decoded outputs and verbatim
 * raw cells for scanned columns — lazy_column.rs:242-256).
 *
 * There is NO CPU compute fallback: every entry point that computes requires
 * a HIP device and fails with COPR_ERR_NO_GPU otherwise.
 */
#include <hip/hip_runtime.h>
#include "../../include/copr_gpu.h"
#include "copr_internal.h"
#include "prod_decimal.h"

#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>

using namespace copr;

static thread_local std::string g_err;
extern "C" const char *copr_last_error(void) { return g_err.c_str(); }
namespace copr {
std::string &tls_err() { return g_err; }   /* shared with copr_comm.cpp */
}

#define SET_ERR(st, msg) (g_err = (msg), (st))
#define HIP_TRY(expr, what)                                                  \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      g_err = std::string(what) + ": " + hipGetErrorString(_e);              \
      return (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice)         \
                 ? COPR_ERR_NO_GPU : COPR_ERR_INTERNAL;                      \
    }                                                                        \
  } while (0)

/* struct copr_engine / copr_region now live in copr_internal.h (shared with
   copr_comm.cpp, the RCCL merge module). */

/* ---------------- engine ---------------- */
extern "C" copr_status copr_engine_create(int hip_device, copr_engine **out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return SET_ERR(COPR_ERR_NO_GPU, "no HIP device available");
  if (hip_device >= n)
    return SET_ERR(COPR_ERR_NO_GPU, "device index out of range");
  HIP_TRY(hipSetDevice(hip_device), "hipSetDevice");
  copr_engine *eng = new copr_engine();
  eng->device = hip_device;
  hipError_t se = hipStreamCreate(&eng->stream);
  if (se != hipSuccess) {
    delete eng;
    return SET_ERR(COPR_ERR_INTERNAL, "hipStreamCreate failed");
  }
  *out = eng;
  return COPR_OK;
}

extern "C" void copr_engine_destroy(copr_engine *eng) {
  if (!eng) return;
  copr::comm_free(eng);
  if (eng->d_crc_tables) hipFree(eng->d_crc_tables);
  {
    copr::HashAggTable &c = eng->ht_cache;
    hipFree(c.keys); hipFree(c.accs); hipFree(c.reserved);
    hipFree(c.ext); hipFree(c.rsvd_ext);
    hipFree(c.rsvd_seen); hipFree(c.error); hipFree(c.n_groups);
  }
  hipFree(eng->d_simple_acc);
  hipFree(eng->d_simple_ext);
  hipFree(eng->d_fcn_state);
  if (eng->h_fcn_out) hipHostFree(eng->h_fcn_out);
  if (eng->stream) hipStreamDestroy(eng->stream);
  delete eng;
}

extern "C" uint64_t copr_engine_plane_launches(const copr_engine *eng) {
  return eng ? eng->plane_launches : 0;
}

extern "C" uint64_t copr_engine_plane_builds(const copr_engine *eng) {
  return eng ? eng->plane_builds : 0;
}

extern "C" uint64_t copr_engine_hash_plane_launches(const copr_engine *eng) {
  return eng ? eng->hash_plane_launches : 0;
}

extern "C" uint64_t copr_engine_narrow_launches(const copr_engine *eng) {
  return eng ? eng->narrow_launches : 0;
}

extern "C" uint64_t copr_engine_narrow_builds(const copr_engine *eng) {
  return eng ? eng->narrow_builds : 0;
}

extern "C" uint64_t copr_engine_split_launches(const copr_engine *eng) {
  return eng ? eng->split_launches : 0;
}

extern "C" uint64_t copr_engine_topn_multi_runs(const copr_engine *eng) {
  return eng ? eng->topn_multi_runs : 0;
}

extern "C" uint64_t copr_engine_topn_last_kept(const copr_engine *eng) {
  return eng ? eng->topn_last_kept : 0;
}

extern "C" uint64_t copr_engine_group_multi_runs(const copr_engine *eng) {
  return eng ? eng->group_multi_runs : 0;
}

extern "C" uint64_t copr_engine_group_last_groups(const copr_engine *eng) {
  return eng ? eng->group_last_groups : 0;
}

extern "C" uint64_t copr_engine_group_dict_grows(const copr_engine *eng) {
  return eng ? eng->group_dict_grows : 0;
}

extern "C" uint64_t copr_engine_group_row_source_runs(const copr_engine *eng) {
  return eng ? eng->group_row_source_runs : 0;
}

extern "C" uint64_t copr_engine_topn_last_candidates(const copr_engine *eng) {
  return eng ? eng->topn_last_candidates : 0;
}

/* ---------------- region ---------------- */
extern "C" copr_status copr_region_create(copr_engine *eng,
                                          const uint8_t *keys, const uint64_t *key_offs,
                                          const uint8_t *vals, const uint64_t *val_offs,
                                          uint64_t n_kv, copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  copr_region *r = new copr_region();
  r->eng = eng;
  r->dev.n_kv = n_kv;
  r->dev.key_bytes = key_offs[n_kv];
  r->dev.val_bytes = val_offs[n_kv];
  uint32_t max_row = 0, max_key = 0;
  for (uint64_t i = 0; i < n_kv; i++) {
    uint64_t l = val_offs[i + 1] - val_offs[i];
    if (l > max_row) max_row = (uint32_t)l;
    uint64_t kl = key_offs[i + 1] - key_offs[i];
    if (kl > max_key) max_key = (uint32_t)kl;
  }
  r->dev.max_row_bytes = max_row;
  r->dev.max_key_bytes = max_key;
  r->h_key_offs.assign(key_offs, key_offs + n_kv + 1);
  r->h_val_offs.assign(val_offs, val_offs + n_kv + 1);

  /* +2 KiB slack: LDS staging reads 16B-aligned past the end, and the glds
     pipeline streams whole 1 KiB chunks */
  auto alloc_copy = [&](void **dst, const void *src, uint64_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(dst, bytes + 2048);
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = alloc_copy((void **)&r->dev.d_keys, keys, r->dev.key_bytes);
  if (e == hipSuccess) e = alloc_copy((void **)&r->dev.d_key_offs, key_offs, (n_kv + 1) * 8);
  if (e == hipSuccess) e = alloc_copy((void **)&r->dev.d_vals, vals, r->dev.val_bytes);
  if (e == hipSuccess) e = alloc_copy((void **)&r->dev.d_val_offs, val_offs, (n_kv + 1) * 8);
  if (e != hipSuccess) {
    g_err = std::string("region upload: ") + hipGetErrorString(e);
    copr_region_destroy(r);
    return e == hipErrorOutOfMemory ? COPR_ERR_OOM : COPR_ERR_INTERNAL;
  }
  if (!getenv("COPR_NO_DIR")) dev_celldir_build(r->dev, eng->stream);
  *out = r;
  return COPR_OK;
}



/* ---- block compression (host side; RocksDB util/compression.h framing,
 * compress_format_version 2: varint32 decompressed size prefix) ---- */
#include <dlfcn.h>

namespace {
typedef int (*lz4_c_fn)(const char *, char *, int, int);
typedef int (*lz4_d_fn)(const char *, char *, int, int);
typedef size_t (*zstd_bound_fn)(size_t);
typedef size_t (*zstd_c_fn)(void *, size_t, const void *, size_t, int);
typedef size_t (*zstd_d_fn)(void *, size_t, const void *, size_t);
typedef unsigned (*zstd_err_fn)(size_t);

struct CompLibs {
  lz4_c_fn lz4_compress = nullptr;
  lz4_d_fn lz4_decompress = nullptr;
  zstd_bound_fn zstd_bound = nullptr;
  zstd_c_fn zstd_compress = nullptr;
  zstd_d_fn zstd_decompress = nullptr;
  zstd_err_fn zstd_iserr = nullptr;
};

static CompLibs *comp_libs() {
  static CompLibs libs;
  static bool tried = false;
  if (!tried) {
    tried = true;
    if (void *l4 = dlopen("liblz4.so.1", RTLD_NOW)) {
      libs.lz4_compress = (lz4_c_fn)dlsym(l4, "LZ4_compress_default");
      libs.lz4_decompress = (lz4_d_fn)dlsym(l4, "LZ4_decompress_safe");
    }
    if (void *lz = dlopen("libzstd.so.1", RTLD_NOW)) {
      libs.zstd_bound = (zstd_bound_fn)dlsym(lz, "ZSTD_compressBound");
      libs.zstd_compress = (zstd_c_fn)dlsym(lz, "ZSTD_compress");
      libs.zstd_decompress = (zstd_d_fn)dlsym(lz, "ZSTD_decompress");
      libs.zstd_iserr = (zstd_err_fn)dlsym(lz, "ZSTD_isError");
    }
  }
  return &libs;
}

static void put_var32(std::vector<uint8_t> *out, uint32_t v) {
  while (v >= 0x80) { out->push_back((uint8_t)(v | 0x80)); v >>= 7; }
  out->push_back((uint8_t)v);
}

static bool get_var32(const uint8_t *p, size_t rem, uint32_t *v, size_t *n) {
  uint32_t x = 0;
  size_t i = 0;
  int sh = 0;
  while (i < rem && i < 5) {
    uint8_t b = p[i++];
    x |= (uint32_t)(b & 0x7F) << sh;
    sh += 7;
    if (!(b & 0x80)) { *v = x; *n = i; return true; }
  }
  return false;
}

static copr_status decompress_blocks(const uint8_t *blocks,
                                     const uint64_t *block_offs,
                                     const uint8_t *types, uint32_t n_blocks,
                                     std::vector<uint8_t> *out,
                                     std::vector<uint64_t> *out_offs) {
  CompLibs *L = comp_libs();
  out_offs->assign(1, 0);
  for (uint32_t b = 0; b < n_blocks; b++) {
    const uint8_t *p = blocks + block_offs[b];
    size_t len = (size_t)(block_offs[b + 1] - block_offs[b]);
    uint8_t t = types ? types[b] : 0;
    if (t == 0) {
      out->insert(out->end(), p, p + len);
    } else if (t == 4 || t == 5 || t == 7) {
      uint32_t raw;
      size_t n;
      if (!get_var32(p, len, &raw, &n))
        return SET_ERR(COPR_ERR_STORAGE, "bad compressed block header");
      size_t base = out->size();
      out->resize(base + raw);
      if (t == 7) {
        if (!L->zstd_decompress)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "libzstd unavailable");
        size_t r = L->zstd_decompress(out->data() + base, raw, p + n,
                                      len - n);
        if (L->zstd_iserr(r) || r != raw)
          return SET_ERR(COPR_ERR_STORAGE, "zstd decompress failed");
      } else {
        if (!L->lz4_decompress)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "liblz4 unavailable");
        int r = L->lz4_decompress((const char *)(p + n),
                                  (char *)(out->data() + base), (int)(len - n),
                                  (int)raw);
        if (r < 0 || (uint32_t)r != raw)
          return SET_ERR(COPR_ERR_STORAGE, "lz4 decompress failed");
      }
    } else {
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "compression type not available (snappy/zlib absent)");
    }
    out_offs->push_back(out->size());
  }
  return COPR_OK;
}
}  // namespace

extern "C" copr_status copr_blocks_decompress(const uint8_t *blocks,
                                              const uint64_t *block_offs,
                                              const uint8_t *types,
                                              uint32_t n_blocks,
                                              uint8_t **out,
                                              uint64_t **out_offs) {
  std::vector<uint8_t> dec;
  std::vector<uint64_t> offs;
  copr_status st = decompress_blocks(blocks, block_offs, types, n_blocks,
                                     &dec, &offs);
  if (st != COPR_OK) return st;
  *out = (uint8_t *)malloc(dec.size() ? dec.size() : 1);
  memcpy(*out, dec.data(), dec.size());
  *out_offs = (uint64_t *)malloc(offs.size() * 8);
  memcpy(*out_offs, offs.data(), offs.size() * 8);
  return COPR_OK;
}

extern "C" copr_status copr_blocks_compress(const uint8_t *blocks,
                                            const uint64_t *block_offs,
                                            uint32_t n_blocks, uint8_t type,
                                            uint8_t **out,
                                            uint64_t **out_offs) {
  CompLibs *L = comp_libs();
  std::vector<uint8_t> all;
  std::vector<uint64_t> offs{0};
  for (uint32_t b = 0; b < n_blocks; b++) {
    const uint8_t *p = blocks + block_offs[b];
    size_t len = (size_t)(block_offs[b + 1] - block_offs[b]);
    std::vector<uint8_t> one;
    put_var32(&one, (uint32_t)len);
    if (type == 4 || type == 5) {
      if (!L->lz4_compress)
        return SET_ERR(COPR_ERR_UNSUPPORTED, "liblz4 unavailable");
      size_t hdr = one.size();
      one.resize(hdr + len + len / 255 + 16);
      int r = L->lz4_compress((const char *)p, (char *)(one.data() + hdr),
                              (int)len, (int)(one.size() - hdr));
      if (r <= 0) return SET_ERR(COPR_ERR_INTERNAL, "lz4 compress failed");
      one.resize(hdr + r);
    } else if (type == 7) {
      if (!L->zstd_compress)
        return SET_ERR(COPR_ERR_UNSUPPORTED, "libzstd unavailable");
      size_t hdr = one.size();
      size_t bound = L->zstd_bound(len);
      one.resize(hdr + bound);
      size_t r = L->zstd_compress(one.data() + hdr, bound, p, len, 3);
      if (L->zstd_iserr(r))
        return SET_ERR(COPR_ERR_INTERNAL, "zstd compress failed");
      one.resize(hdr + r);
    } else {
      return SET_ERR(COPR_ERR_UNSUPPORTED, "compression type");
    }
    all.insert(all.end(), one.begin(), one.end());
    offs.push_back(all.size());
  }
  *out = (uint8_t *)malloc(all.size() ? all.size() : 1);
  memcpy(*out, all.data(), all.size());
  *out_offs = (uint64_t *)malloc(offs.size() * 8);
  memcpy(*out_offs, offs.data(), offs.size() * 8);
  return COPR_OK;
}

extern "C" copr_status copr_region_create_blocks_compressed(
    copr_engine *eng, const uint8_t *blocks, const uint64_t *block_offs,
    const uint8_t *types, uint32_t n_blocks, copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  std::vector<uint8_t> dec;
  std::vector<uint64_t> offs;
  copr_status st = decompress_blocks(blocks, block_offs, types, n_blocks,
                                     &dec, &offs);
  if (st != COPR_OK) return st;
  return copr_region_create_blocks(eng, dec.data(), offs.data(), n_blocks,
                                   out);
}


/* ---- SST data-block ingestion (copr_gpu.h) ---- */
static copr_status region_from_dev(copr_engine *eng, DevRegion dr,
                                   copr_region **out) {
  copr_region *r = new copr_region();
  r->eng = eng;
  r->dev = dr;
  r->h_key_offs.resize(dr.n_kv + 1);
  r->h_val_offs.resize(dr.n_kv + 1);
  hipError_t ce = hipMemcpy(r->h_key_offs.data(), dr.d_key_offs,
                            (dr.n_kv + 1) * 8, hipMemcpyDeviceToHost);
  if (ce == hipSuccess)
    ce = hipMemcpy(r->h_val_offs.data(), dr.d_val_offs, (dr.n_kv + 1) * 8,
                   hipMemcpyDeviceToHost);
  if (ce != hipSuccess) {
    copr_region_destroy(r);
    return SET_ERR(COPR_ERR_INTERNAL, "region offs readback");
  }
  uint32_t mr = 0, mk = 0;
  for (uint64_t i = 0; i < dr.n_kv; i++) {
    uint64_t l = r->h_val_offs[i + 1] - r->h_val_offs[i];
    if (l > mr) mr = (uint32_t)l;
    uint64_t kl = r->h_key_offs[i + 1] - r->h_key_offs[i];
    if (kl > mk) mk = (uint32_t)kl;
  }
  r->dev.max_row_bytes = mr;
  r->dev.max_key_bytes = mk;
  if (!getenv("COPR_NO_DIR")) dev_celldir_build(r->dev, eng->stream);
  *out = r;
  return COPR_OK;
}

extern "C" copr_status copr_region_create_blocks(copr_engine *eng,
                                                 const uint8_t *blocks,
                                                 const uint64_t *block_offs,
                                                 uint32_t n_blocks,
                                                 copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  DevRegion dr{};
  int rc = dev_blocks_build(blocks, block_offs, n_blocks, &dr, eng->stream);
  if (rc == -3) return SET_ERR(COPR_ERR_STORAGE, "malformed data block");
  if (rc == -2) return SET_ERR(COPR_ERR_OOM, "block ingest alloc");
  if (rc != 0) return SET_ERR(COPR_ERR_INTERNAL, "block ingest failed");
  return region_from_dev(eng, dr, out);
}

extern "C" copr_status copr_region_create_blocks_mvcc(
    copr_engine *eng, const uint8_t *blocks, const uint64_t *block_offs,
    uint32_t n_blocks, uint64_t read_ts, copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  DevRegion raw{};
  int rc = dev_blocks_build(blocks, block_offs, n_blocks, &raw, eng->stream);
  if (rc == -3) return SET_ERR(COPR_ERR_STORAGE, "malformed data block");
  if (rc == -2) return SET_ERR(COPR_ERR_OOM, "block ingest alloc");
  if (rc != 0) return SET_ERR(COPR_ERR_INTERNAL, "block ingest failed");
  DevRegion vis{};
  int unsup = 0;
  rc = dev_mvcc_build(raw.d_keys, raw.d_key_offs, raw.d_vals, raw.d_val_offs,
                      raw.n_kv, nullptr, nullptr, nullptr, nullptr, 0,
                      read_ts, &vis, &unsup, eng->stream);
  hipFree(raw.d_keys); hipFree(raw.d_key_offs);
  hipFree(raw.d_vals); hipFree(raw.d_val_offs);
  if (rc == -3) return SET_ERR(COPR_ERR_UNSUPPORTED, "mvcc: default-CF value");
  if (rc == -2) return SET_ERR(COPR_ERR_OOM, "mvcc build oom");
  if (rc != 0) return SET_ERR(COPR_ERR_STORAGE, "malformed write-CF entry");
  return region_from_dev(eng, vis, out);
}

/* ---- whole-SST ingestion (file layer) ----
 * RocksDB BlockBasedTable reader restated from the public format
 * (format.cc / block_based_table_reader.cc; TiKV reads SSTs through
 * rust-rocksdb iterators, engine_iterator.rs:12):
 *   footer (format_version 1..5, last 53 bytes):
 *     [checksum_type u8][metaindex BlockHandle][index BlockHandle]
 *     [zero padding to 40 handle bytes][format_version u32le][magic u64le]
 *   every block on disk: [contents][compression_type u8][checksum u32le]
 *   checksum = RocksDB-masked crc32c(contents || type byte) when
 *   checksum_type == 1 (kCRC32c, the TiKV default); other checksum kinds
 *   (xxHash family) are accepted but not verified.
 *   index block: standard block entries whose values are BlockHandles
 *   ([varint64 offset][varint64 size]; kBinarySearch, no delta encoding —
 *   the TiKV-written shape). format_version 0 (pre-2014 legacy footer)
 *   and >= 6 (self-checksummed footer) are rejected loudly. */
namespace {

static const uint64_t kSstMagic = 0x88e241b785f4cff7ull;

static uint32_t crc32c_tab[8][256];
static void crc32c_init_once() {
  static bool done = false;
  if (done) return;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0x82F63B78u : 0);
    crc32c_tab[0][i] = c;
  }
  for (int t = 1; t < 8; t++)
    for (uint32_t i = 0; i < 256; i++)
      crc32c_tab[t][i] = crc32c_tab[0][crc32c_tab[t - 1][i] & 0xFF] ^
                         (crc32c_tab[t - 1][i] >> 8);
  done = true;
}

static uint32_t crc32c(const uint8_t *p, size_t n) {
  crc32c_init_once();
  uint32_t c = 0xFFFFFFFFu;
  while (n >= 8) {
    uint32_t lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                  ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    lo ^= c;
    c = crc32c_tab[7][lo & 0xFF] ^ crc32c_tab[6][(lo >> 8) & 0xFF] ^
        crc32c_tab[5][(lo >> 16) & 0xFF] ^ crc32c_tab[4][lo >> 24] ^
        crc32c_tab[3][p[4]] ^ crc32c_tab[2][p[5]] ^
        crc32c_tab[1][p[6]] ^ crc32c_tab[0][p[7]];
    p += 8; n -= 8;
  }
  while (n--) c = crc32c_tab[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

static inline uint32_t crc32c_mask(uint32_t crc) {
  return ((crc >> 15) | (crc << 17)) + 0xa282ead8u;   /* util/crc32c.h */
}

static bool get_var64(const uint8_t *p, size_t rem, uint64_t *v, size_t *n) {
  uint64_t x = 0;
  size_t i = 0;
  int sh = 0;
  while (i < rem && i < 10) {
    uint8_t b = p[i++];
    x |= (uint64_t)(b & 0x7F) << sh;
    sh += 7;
    if (!(b & 0x80)) { *v = x; *n = i; return true; }
  }
  return false;
}

struct SstBlockRef { uint64_t off, size; uint8_t type; };

/* checks the 5-byte trailer; returns the compression type byte */
static copr_status sst_block_trailer(const uint8_t *f, uint64_t len,
                                     uint64_t off, uint64_t size,
                                     uint8_t cks_type, uint8_t *type) {
  if (off + size + 5 > len)
    return SET_ERR(COPR_ERR_STORAGE, "SST block handle out of bounds");
  *type = f[off + size];
  if (cks_type == 1) {
    uint32_t stored = (uint32_t)f[off + size + 1] |
                      ((uint32_t)f[off + size + 2] << 8) |
                      ((uint32_t)f[off + size + 3] << 16) |
                      ((uint32_t)f[off + size + 4] << 24);
    if (crc32c_mask(crc32c(f + off, size + 1)) != stored)
      return SET_ERR(COPR_ERR_STORAGE, "SST block checksum mismatch");
  }
  return COPR_OK;
}

static copr_status sst_layout(const uint8_t *f, uint64_t len,
                              std::vector<SstBlockRef> *blocks) {
  if (len < 53) return SET_ERR(COPR_ERR_STORAGE, "SST too short");
  uint64_t magic = 0;
  for (int i = 7; i >= 0; i--) magic = (magic << 8) | f[len - 8 + i];
  if (magic != kSstMagic)
    return SET_ERR(COPR_ERR_STORAGE, "not a BlockBasedTable SST (bad magic)");
  uint32_t ver = (uint32_t)f[len - 12] | ((uint32_t)f[len - 11] << 8) |
                 ((uint32_t)f[len - 10] << 16) | ((uint32_t)f[len - 9] << 24);
  if (ver < 1 || ver > 5)
    return SET_ERR(COPR_ERR_UNSUPPORTED,
                   "SST format_version outside 1..5 (legacy and v6+ footers "
                   "unsupported)");
  const uint8_t *fp = f + (len - 53);
  uint8_t cks_type = fp[0];
  const uint8_t *hp = fp + 1;
  size_t hrem = 40, n = 0;
  uint64_t m_off, m_sz, i_off, i_sz;
  if (!get_var64(hp, hrem, &m_off, &n)) goto badfoot;
  hp += n; hrem -= n;
  if (!get_var64(hp, hrem, &m_sz, &n)) goto badfoot;
  hp += n; hrem -= n;
  if (!get_var64(hp, hrem, &i_off, &n)) goto badfoot;
  hp += n; hrem -= n;
  if (!get_var64(hp, hrem, &i_sz, &n)) goto badfoot;
  (void)m_off; (void)m_sz;                 /* metaindex: not consulted */
  {
    uint8_t itype = 0;
    copr_status st = sst_block_trailer(f, len, i_off, i_sz, cks_type, &itype);
    if (st != COPR_OK) return st;
    std::vector<uint8_t> idec;
    const uint8_t *ib = f + i_off;
    size_t iblen = (size_t)i_sz;
    if (itype != 0) {
      std::vector<uint64_t> one_offs{0, i_sz};
      std::vector<uint64_t> dof;
      std::vector<uint8_t> ty{itype};
      st = decompress_blocks(f + i_off, one_offs.data(), ty.data(), 1,
                             &idec, &dof);
      if (st != COPR_OK) return st;
      ib = idec.data();
      iblen = idec.size();
    }
    /* walk the index entries; values are BlockHandles */
    if (iblen < 8) return SET_ERR(COPR_ERR_STORAGE, "SST index block short");
    uint32_t nr = (uint32_t)ib[iblen - 4] | ((uint32_t)ib[iblen - 3] << 8) |
                  ((uint32_t)ib[iblen - 2] << 16) |
                  ((uint32_t)ib[iblen - 1] << 24);
    if (iblen < 4 + (size_t)nr * 4)
      return SET_ERR(COPR_ERR_STORAGE, "SST index restart array");
    size_t data_end = iblen - 4 - (size_t)nr * 4;
    std::string key;
    size_t pos = 0;
    while (pos < data_end) {
      uint32_t shared, non_shared, vlen;
      size_t vn;
      if (!get_var32(ib + pos, data_end - pos, &shared, &vn)) goto badidx;
      pos += vn;
      if (!get_var32(ib + pos, data_end - pos, &non_shared, &vn)) goto badidx;
      pos += vn;
      if (!get_var32(ib + pos, data_end - pos, &vlen, &vn)) goto badidx;
      pos += vn;
      if (pos + non_shared + vlen > data_end || shared > key.size())
        goto badidx;
      key.resize(shared);
      key.append((const char *)(ib + pos), non_shared);
      pos += non_shared;
      uint64_t b_off, b_sz;
      size_t hn1, hn2;
      if (!get_var64(ib + pos, vlen, &b_off, &hn1) ||
          !get_var64(ib + pos + hn1, vlen - hn1, &b_sz, &hn2))
        return SET_ERR(COPR_ERR_UNSUPPORTED,
                       "SST index value is not a plain BlockHandle");
      pos += vlen;
      uint8_t btype = 0;
      copr_status bs = sst_block_trailer(f, len, b_off, b_sz, cks_type,
                                         &btype);
      if (bs != COPR_OK) return bs;
      blocks->push_back({b_off, b_sz, btype});
    }
    if (pos != data_end) goto badidx;
  }
  if (blocks->empty())
    return SET_ERR(COPR_ERR_STORAGE, "SST has no data blocks");
  return COPR_OK;
badfoot:
  return SET_ERR(COPR_ERR_STORAGE, "SST footer handles malformed");
badidx:
  return SET_ERR(COPR_ERR_STORAGE, "SST index block malformed");
}

/* slices + decompresses every data block into one uncompressed
   concatenation (the shape the device block parser ingests) */
static copr_status sst_collect(const uint8_t *f, uint64_t len,
                               std::vector<uint8_t> *dec,
                               std::vector<uint64_t> *doffs,
                               uint32_t *n_blocks) {
  std::vector<SstBlockRef> refs;
  copr_status st = sst_layout(f, len, &refs);
  if (st != COPR_OK) return st;
  std::vector<uint8_t> cat;
  std::vector<uint64_t> offs{0};
  std::vector<uint8_t> types;
  for (const SstBlockRef &r : refs) {
    cat.insert(cat.end(), f + r.off, f + r.off + r.size);
    offs.push_back(cat.size());
    types.push_back(r.type);
  }
  st = decompress_blocks(cat.data(), offs.data(), types.data(),
                         (uint32_t)refs.size(), dec, doffs);
  if (st != COPR_OK) return st;
  *n_blocks = (uint32_t)refs.size();
  return COPR_OK;
}

}  // namespace

extern "C" copr_status copr_region_create_sst(copr_engine *eng,
                                              const uint8_t *file,
                                              uint64_t file_len,
                                              copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  std::vector<uint8_t> dec;
  std::vector<uint64_t> doffs;
  uint32_t nb = 0;
  copr_status st = sst_collect(file, file_len, &dec, &doffs, &nb);
  if (st != COPR_OK) return st;
  return copr_region_create_blocks(eng, dec.data(), doffs.data(), nb, out);
}

extern "C" copr_status copr_region_create_sst_mvcc(copr_engine *eng,
                                                   const uint8_t *file,
                                                   uint64_t file_len,
                                                   uint64_t read_ts,
                                                   copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  std::vector<uint8_t> dec;
  std::vector<uint64_t> doffs;
  uint32_t nb = 0;
  copr_status st = sst_collect(file, file_len, &dec, &doffs, &nb);
  if (st != COPR_OK) return st;
  return copr_region_create_blocks_mvcc(eng, dec.data(), doffs.data(), nb,
                                        read_ts, out);
}

static copr_status region_create_mvcc_impl(copr_engine *eng,
                                           const uint8_t *keys,
                                           const uint64_t *key_offs,
                                           const uint8_t *vals,
                                           const uint64_t *val_offs,
                                           uint64_t n_kv,
                                           const uint8_t *dkeys,
                                           const uint64_t *dkey_offs,
                                           const uint8_t *dvals,
                                           const uint64_t *dval_offs,
                                           uint64_t n_default,
                                           uint64_t read_ts,
                                           copr_region **out) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  /* upload raw write-CF (+ optional default-CF) arrays (temporary) */
  uint8_t *rk = nullptr, *rv = nullptr;
  uint64_t *rko = nullptr, *rvo = nullptr;
  uint8_t *dk = nullptr, *dv = nullptr;
  uint64_t *dko = nullptr, *dvo = nullptr;
  hipError_t e = hipSuccess;
  auto up = [&](void **dst, const void *srcp, uint64_t bytes) {
    if (e != hipSuccess) return;
    e = hipMalloc(dst, bytes + 2048);
    if (e == hipSuccess) e = hipMemcpy(*dst, srcp, bytes, hipMemcpyHostToDevice);
  };
  up((void **)&rk, keys, key_offs[n_kv]);
  up((void **)&rko, key_offs, (n_kv + 1) * 8);
  up((void **)&rv, vals, val_offs[n_kv]);
  up((void **)&rvo, val_offs, (n_kv + 1) * 8);
  if (dkeys) {
    up((void **)&dk, dkeys, dkey_offs[n_default]);
    up((void **)&dko, dkey_offs, (n_default + 1) * 8);
    up((void **)&dv, dvals, dval_offs[n_default]);
    up((void **)&dvo, dval_offs, (n_default + 1) * 8);
  }
  auto free_raw = [&]() {
    hipFree(rk); hipFree(rko); hipFree(rv); hipFree(rvo);
    hipFree(dk); hipFree(dko); hipFree(dv); hipFree(dvo);
  };
  if (e != hipSuccess) {
    free_raw();
    return SET_ERR(e == hipErrorOutOfMemory ? COPR_ERR_OOM : COPR_ERR_INTERNAL,
                   "mvcc upload failed");
  }
  DevRegion dr{};
  int unsup = 0;
  int rc = dev_mvcc_build(rk, rko, rv, rvo, n_kv, dk, dko, dv, dvo, n_default,
                          read_ts, &dr, &unsup, eng->stream);
  free_raw();
  if (rc == -3) return SET_ERR(COPR_ERR_UNSUPPORTED, "mvcc: default-CF value");
  if (rc == -2) return SET_ERR(COPR_ERR_OOM, "mvcc build oom");
  if (rc != 0) return SET_ERR(COPR_ERR_STORAGE, "malformed write-CF entry");
  copr_region *r = new copr_region();
  r->eng = eng;
  r->dev = dr;
  r->h_key_offs.resize(dr.n_kv + 1);
  r->h_val_offs.resize(dr.n_kv + 1);
  hipError_t ce = hipMemcpy(r->h_key_offs.data(), dr.d_key_offs,
                            (dr.n_kv + 1) * 8, hipMemcpyDeviceToHost);
  if (ce == hipSuccess)
    ce = hipMemcpy(r->h_val_offs.data(), dr.d_val_offs, (dr.n_kv + 1) * 8,
                   hipMemcpyDeviceToHost);
  if (ce != hipSuccess) {
    copr_region_destroy(r);
    return SET_ERR(COPR_ERR_INTERNAL, "mvcc offs readback");
  }
  if (!getenv("COPR_NO_DIR")) dev_celldir_build(r->dev, eng->stream);
  *out = r;
  return COPR_OK;
}

extern "C" copr_status copr_region_create_mvcc(copr_engine *eng,
                                               const uint8_t *keys,
                                               const uint64_t *key_offs,
                                               const uint8_t *vals,
                                               const uint64_t *val_offs,
                                               uint64_t n_kv, uint64_t read_ts,
                                               copr_region **out) {
  return region_create_mvcc_impl(eng, keys, key_offs, vals, val_offs, n_kv,
                                 nullptr, nullptr, nullptr, nullptr, 0,
                                 read_ts, out);
}

extern "C" copr_status copr_region_create_mvcc_with_default(
    copr_engine *eng, const uint8_t *keys, const uint64_t *key_offs,
    const uint8_t *vals, const uint64_t *val_offs, uint64_t n_kv,
    const uint8_t *dkeys, const uint64_t *dkey_offs, const uint8_t *dvals,
    const uint64_t *dval_offs, uint64_t n_default, uint64_t read_ts,
    copr_region **out) {
  if (!dkeys || !dkey_offs || !dvals || !dval_offs)
    return SET_ERR(COPR_ERR_INVALID_REQUEST, "null default-CF stream");
  return region_create_mvcc_impl(eng, keys, key_offs, vals, val_offs, n_kv,
                                 dkeys, dkey_offs, dvals, dval_offs,
                                 n_default, read_ts, out);
}

extern "C" copr_status copr_region_dump(copr_engine *eng, copr_region *r,
                                        CoprGenOut *out) {
  if (!eng || !r) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null arg");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  memset(out, 0, sizeof(*out));
  uint64_t n = r->dev.n_kv;
  out->n_kv = n;
  out->keys = (uint8_t *)malloc(r->dev.key_bytes + 1);
  out->vals = (uint8_t *)malloc(r->dev.val_bytes + 1);
  out->key_offs = (uint64_t *)malloc((n + 1) * 8);
  out->val_offs = (uint64_t *)malloc((n + 1) * 8);
  if (!out->keys || !out->vals || !out->key_offs || !out->val_offs)
    return SET_ERR(COPR_ERR_OOM, "dump alloc");
  HIP_TRY(hipMemcpy(out->keys, r->dev.d_keys, r->dev.key_bytes,
                    hipMemcpyDeviceToHost), "dump keys");
  HIP_TRY(hipMemcpy(out->vals, r->dev.d_vals, r->dev.val_bytes,
                    hipMemcpyDeviceToHost), "dump vals");
  HIP_TRY(hipMemcpy(out->key_offs, r->dev.d_key_offs, (n + 1) * 8,
                    hipMemcpyDeviceToHost), "dump koffs");
  HIP_TRY(hipMemcpy(out->val_offs, r->dev.d_val_offs, (n + 1) * 8,
                    hipMemcpyDeviceToHost), "dump voffs");
  return COPR_OK;
}

extern "C" void copr_region_destroy(copr_region *r) {
  if (!r) return;
  hipFree(r->dev.d_keys); hipFree(r->dev.d_key_offs);
  hipFree(r->dev.d_vals); hipFree(r->dev.d_val_offs);
  if (r->dev.d_celldir) hipFree(r->dev.d_celldir);
  dev_colplane_free(r->dev);
  delete r;
}

extern "C" uint64_t copr_region_num_kv(const copr_region *r) { return r ? r->dev.n_kv : 0; }

/* ---------------- planning ---------------- */
namespace {

struct HostPlan {
  ScanPlan sp{};
  int filter_col_offset = -1;
  /* scan schema */
  std::vector<CoprColumnInfo> cols;
  std::vector<CoprFieldType> out_schema;
  /* agg bookkeeping: response column layout */
  struct OutAgg { int32_t func; int dev_idx; CoprFieldType out_ft; int in_kind; };
  std::vector<OutAgg> out_aggs;
  bool has_agg = false;
  bool hash_agg = false;
  bool stream_agg = false;
  bool simple_as_stream = false;   /* simple agg with FIRST: one-run stream */
  bool hash_sorted = false;        /* FastHash + FIRST: sorted pipeline */
  CoprFieldType group_ft{};
  /* several group-by columns: group_multi with the distinct key
     columns in group_keys; group_pos[j] = the key that output group column j
     (request order, repeats included) shows */
  bool group_multi = false;
  std::vector<copr::GroupKey> group_keys;
  std::vector<int> group_pos;
  /* TopN (top_n_executor.rs): int order-by columns. One order-by
     expression: topn_off / topn_desc and dev_topn_select. Several (DESIGN
     §9f): topn_multi with the distinct keys in topn_keys. */
  bool has_topn = false;
  uint64_t topn_n = 0;
  int topn_desc = 0;
  int topn_off = -1;
  bool topn_multi = false;
  std::vector<copr::TopnKey> topn_keys;
  int dec2_col_offset = -1;
  int filter2_col_offset = -1;
  /* offsets of the third and fourth column an RPN selection names (the
     extra-capture channels), -1 = none */
  int xcap_col_offset[2] = {-1, -1};
  uint64_t limit = UINT64_MAX;
};

static bool et_int(int32_t tp) {
  switch (tp) {
    case COPR_TP_TINY: case COPR_TP_SHORT: case COPR_TP_INT24:
    case COPR_TP_LONG: case COPR_TP_LONGLONG: case COPR_TP_YEAR: return true;
    default: return false;
  }
}

/* decode an int datum (flag+payload) on host — used for default values.
 * Mirrors decode_int_datum (datum_codec.rs:401-420). Returns 0 ok/1 null/-1 err. */
static int host_decode_int_datum(const uint8_t *p, size_t len, int64_t *v) {
  if (len == 0) return -1;
  uint8_t flag = p[0];
  p++; len--;
  auto be64 = [](const uint8_t *q) {
    uint64_t x = 0;
    for (int i = 0; i < 8; i++) x = (x << 8) | q[i];
    return x;
  };
  switch (flag) {
    case 0: return 1;
    case 3: if (len < 8) return -1; *v = (int64_t)(be64(p) ^ 0x8000000000000000ull); return 0;
    case 4: if (len < 8) return -1; *v = (int64_t)be64(p); return 0;
    case 8: case 9: {
      uint64_t val = 0;
      int shift = 0;
      size_t i = 0;
      while (i < len && p[i] >= 0x80 && i < 9) {
        val |= (uint64_t)(p[i] & 0x7F) << shift;
        shift += 7; i++;
      }
      if (i >= len) return -1;
      val |= (uint64_t)p[i] << shift;
      if (flag == 8) {
        uint64_t half = val >> 1;
        *v = (val & 1) ? (int64_t)~half : (int64_t)half;
      } else {
        *v = (int64_t)val;
      }
      return 0;
    }
    default: return -1;
  }
}

/* pattern-match a selection condition: cmp(colref_int, const_int) (either
 * operand order). Mirrors LtInt-class dispatch (lib.rs:523, map_int_sig). */
static copr_status match_filter(const CoprExpr &cond, HostPlan &pl, ScanPlan *sp) {
  if (cond.n_nodes != 3) return COPR_ERR_UNSUPPORTED;
  const CoprExprNode &a = cond.nodes[0], &b = cond.nodes[1], &f = cond.nodes[2];
  if (f.kind != COPR_EXPR_SCALAR_FUNC || f.n_args != 2) return COPR_ERR_UNSUPPORTED;
  int cmp;
  bool is_real = false;
  switch (f.sig) {
    case COPR_SIG_LT_INT: cmp = CMP_LT; break;
    case COPR_SIG_LE_INT: cmp = CMP_LE; break;
    case COPR_SIG_GT_INT: cmp = CMP_GT; break;
    case COPR_SIG_GE_INT: cmp = CMP_GE; break;
    case COPR_SIG_EQ_INT: cmp = CMP_EQ; break;
    case COPR_SIG_NE_INT: cmp = CMP_NE; break;
    /* Real comparers (impl_compare.rs:66-160 Real path) */
    case COPR_SIG_LT_REAL: cmp = CMP_LT; is_real = true; break;
    case COPR_SIG_LE_REAL: cmp = CMP_LE; is_real = true; break;
    case COPR_SIG_GT_REAL: cmp = CMP_GT; is_real = true; break;
    case COPR_SIG_GE_REAL: cmp = CMP_GE; is_real = true; break;
    case COPR_SIG_EQ_REAL: cmp = CMP_EQ; is_real = true; break;
    case COPR_SIG_NE_REAL: cmp = CMP_NE; is_real = true; break;
    default: return COPR_ERR_UNSUPPORTED;
  }
  auto const_ok = [&](const CoprExprNode &n) {
    if (n.kind == COPR_EXPR_CONST_NULL) return true;
    if (is_real) return n.kind == COPR_EXPR_CONST_REAL;
    return n.kind == COPR_EXPR_CONST_INT || n.kind == COPR_EXPR_CONST_UINT;
  };
  const CoprExprNode *colref, *konst;
  bool swapped;
  if (a.kind == COPR_EXPR_COLUMN_REF && const_ok(b)) {
    colref = &a; konst = &b; swapped = false;
  } else if (b.kind == COPR_EXPR_COLUMN_REF && const_ok(a)) {
    colref = &b; konst = &a; swapped = true;
  } else {
    return COPR_ERR_UNSUPPORTED;
  }
  size_t off = (size_t)colref->i64_val;
  if (off >= pl.cols.size()) return COPR_ERR_INVALID_REQUEST;
  const CoprColumnInfo &ci = pl.cols[off];
  if (is_real) {
    if (ci.ft.tp != COPR_TP_DOUBLE && ci.ft.tp != COPR_TP_FLOAT)
      return COPR_ERR_UNSUPPORTED;
  } else if (!et_int(ci.ft.tp)) {
    return COPR_ERR_UNSUPPORTED;
  }
  if (ci.pk_handle && !pl.sp.index_mode) return COPR_ERR_UNSUPPORTED;
  if (is_real && pl.sp.index_mode) return COPR_ERR_UNSUPPORTED;
  pl.filter_col_offset = (int)off;
  if (swapped) {
    /* const OP col  ==  col flip(OP) const */
    switch (cmp) {
      case CMP_LT: cmp = CMP_GT; break;
      case CMP_LE: cmp = CMP_GE; break;
      case CMP_GT: cmp = CMP_LT; break;
      case CMP_GE: cmp = CMP_LE; break;
      default: break;
    }
  }
  sp->has_filter = 1;
  sp->filter_col_id = ci.column_id;
  sp->filter_is_real = is_real ? 1 : 0;
  /* default fill for a row missing this column (scan fills defaults before
     the predicate decodes the column) */
  if (ci.default_val && ci.default_val_len) {
    if (is_real) {
      /* FLOAT datum default: flag 5 + 8B comparable f64 -> IEEE bits */
      if (ci.default_val_len != 9 || ci.default_val[0] != 5)
        return COPR_ERR_INVALID_REQUEST;
      uint64_t u = 0;
      for (int b2 = 0; b2 < 8; b2++) u = (u << 8) | ci.default_val[1 + b2];
      sp->filter_missing_val =
          (int64_t)((u & 0x8000000000000000ull) ? (u ^ 0x8000000000000000ull)
                                                : ~u);
      sp->filter_missing_null = 0;
    } else {
      int64_t dv;
      int r = host_decode_int_datum(ci.default_val, ci.default_val_len, &dv);
      if (r < 0) return COPR_ERR_INVALID_REQUEST;
      sp->filter_missing_null = r == 1 ? 1 : 0;
      sp->filter_missing_val = dv;
    }
  } else {
    /* NULLable: missing -> NULL. (A missing NOT NULL column is a data
       error in the reference; rows cannot legally lack it.) */
    sp->filter_missing_null = 1;
  }
  sp->filter_cmp = cmp;
  if (is_real && konst->kind == COPR_EXPR_CONST_REAL) {
    double dv = konst->f64_val;
    memcpy(&sp->filter_const, &dv, 8);           /* f64 BITS */
  } else {
    sp->filter_const = konst->i64_val;
  }
  sp->filter_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
  sp->filter_const_unsigned =
      (konst->kind == COPR_EXPR_CONST_UINT || (konst->ft.flag & COPR_FLAG_UNSIGNED)) ? 1 : 0;
  sp->filter_const_null = konst->kind == COPR_EXPR_CONST_NULL ? 1 : 0;
  return COPR_OK;
}


/* directory usable for the generic collect path? every column the plan
   touches must be a small id with a plane (1..16) */
static void wire_celldir(ScanPlan *sp, const DevRegion &dev) {
  sp->dir_plane = nullptr;
  sp->celldir = nullptr;
  sp->celldir_n = 0;
  sp->n_dir_slabs = 0;
  sp->dirslab_f = sp->dirslab_f2 = sp->dirslab_g = -1;
  for (int a = 0; a < COPR_MAX_AGGS; a++) sp->dirslab_a[a] = -1;
  if (sp->index_mode || !dev.d_celldir) return;
  if (sp->has_filter && sp->filter_col_id >= 1 && sp->filter_col_id <= 16)
    sp->dir_plane = dev.d_celldir +
                    (uint64_t)(sp->filter_col_id - 1) * dev.n_kv;
  bool ok = true;
  if (sp->has_filter && (sp->filter_col_id < 1 || sp->filter_col_id > 16))
    ok = false;
  if (sp->filter2_on && (sp->filter2_col_id < 1 || sp->filter2_col_id > 16))
    ok = false;
  if ((sp->mode == 2 || sp->mode == 3 || sp->mode == 4 ||
       sp->group_col_id != 0) &&
      (sp->group_col_id < 1 || sp->group_col_id > 16))
    ok = false;
  for (int a = 0; a < sp->n_aggs && ok; a++)
    if (sp->aggs[a].kind != DAGG_COUNT_ROWS &&
        (sp->aggs[a].col_id < 1 || sp->aggs[a].col_id > 16))
      ok = false;
  if (ok) { sp->celldir = dev.d_celldir; sp->celldir_n = dev.n_kv; }

  /* assign staged dir slabs (pipe kernel): one per DISTINCT needed plane,
     slab 0 = the filter plane (FASTFC contract) */
  if (!ok && !sp->dir_plane) return;
  auto slab_of = [&](int64_t col) -> int32_t {
    if (col < 1 || col > 16) return -1;
    const uint8_t *p = dev.d_celldir + (uint64_t)(col - 1) * dev.n_kv;
    for (int32_t k = 0; k < sp->n_dir_slabs; k++)
      if (sp->dir_planes_staged[k] == p) return k;
    if (sp->n_dir_slabs == COPR_MAX_DIR_SLABS) return -1;
    sp->dir_planes_staged[sp->n_dir_slabs] = p;
    return sp->n_dir_slabs++;
  };
  if (sp->has_filter) sp->dirslab_f = slab_of(sp->filter_col_id);
  if (sp->filter2_on) sp->dirslab_f2 = slab_of(sp->filter2_col_id);
  if (sp->mode == 2 || sp->group_col_id != 0)
    sp->dirslab_g = slab_of(sp->group_col_id);
  for (int a = 0; a < sp->n_aggs; a++)
    if (sp->aggs[a].kind != DAGG_COUNT_ROWS)
      sp->dirslab_a[a] = slab_of(sp->aggs[a].col_id);
}


/* ---- column planes ----
   Plan-level eligibility: a simple aggregate whose keep decision is at most
   two cmp(col, const) conjuncts and whose aggregates only need a column's
   int value or presence. A plan that references no column at all stays on
   the scan path (it has nothing to read from a plane). */
static bool plane_plan_ok(const ScanPlan &sp) {
  if (sp.mode != 1 || sp.index_mode || sp.rpn_on || sp.n_xcap ||
      sp.filter_decode_only || sp.dec2_col_id)
    return false;
  bool any_col = sp.has_filter || sp.filter2_on;
  for (int a = 0; a < sp.n_aggs; a++) {
    switch (sp.aggs[a].kind) {
      case DAGG_COUNT_ROWS: break;
      case DAGG_COUNT_COL: case DAGG_SUM_INT:
      case DAGG_MAX_INT: case DAGG_MIN_INT: any_col = true; break;
      default: return false;
    }
  }
  return any_col;
}

/* FastHashAgg (int group key) over a table scan with the same
   keep decision, and aggregates that need a column's int or <= 38-digit
   decimal value or its presence. count(NULL) rides a column id that never
   exists and has nothing to read from a plane. */
static bool hash_plane_plan_ok(const ScanPlan &sp) {
  if (sp.mode != 2 || sp.index_mode || sp.rpn_on || sp.n_xcap ||
      sp.filter_decode_only || sp.dec2_col_id || sp.group_col_id <= 0)
    return false;
  for (int a = 0; a < sp.n_aggs; a++) {
    switch (sp.aggs[a].kind) {
      case DAGG_COUNT_ROWS: break;
      case DAGG_COUNT_COL: case DAGG_SUM_INT: case DAGG_SUM_DEC:
      case DAGG_MAX_INT: case DAGG_MIN_INT:
        if (sp.aggs[a].col_id <= 0) return false;
        break;
      default: return false;
    }
  }
  return true;
}

static bool plane_set_used(const PlaneSet &ps) {
  if (ps.g.val || ps.f.val || ps.f2.val) return true;
  for (int a = 0; a < COPR_MAX_AGGS; a++)
    if (ps.a[a].val) return true;
  return false;
}

/* Region-level: wire every column the plan references to a plane of this
   region, building missing ones within the budget. All or nothing: false
   leaves the region on the scan path. A plane records each row as the scan
   path sees it, and that depends on how the scan locates cells: through the
   directory when every referenced id has a directory plane (1..16), by
   walking otherwise. So with a directory present the same id rule as
   wire_celldir applies.
   hash = the k_plane_hash consumer: it also wires the group column, reads
   decimal rows from the plane, and may spend the region's full value bytes
   on planes where the simple consumer stops at half.
   nu (simple consumer only): when the wiring has the k_plane_fc shape, the
   filter plane's narrow companion is built here on first use and the filter
   folded into its domain; nu->p stays null when the region
   keeps k_plane_fc. */
struct NarrowUse {
  const DevRegion::ColPlane *p = nullptr;
  NarrowFcArgs nf{};
  SplitFcArgs sf{};                /* a split plane's form of nf */
};

static bool plane_wire(copr_engine *eng, DevRegion &dev, const ScanPlan &sp,
                       PlaneSet *ps, bool hash = false,
                       NarrowUse *nu = nullptr, bool wire_group = true) {
  *ps = PlaneSet{};
  if (nu) *nu = NarrowUse{};
  if (!dev.n_kv) return false;
  uint64_t budget = hash ? dev.val_bytes : dev.val_bytes / 2;
  if (const char *e = getenv("COPR_PLANE_BUDGET_MB"))
    budget = (uint64_t)strtoull(e, nullptr, 10) << 20;
  struct Want { int64_t col; PlaneRef *ref; };
  Want want[COPR_MAX_AGGS + 3];
  int n_want = 0;
  /* wire_group false: the caller supplies ps->g (multi-key group ids) */
  if (hash && wire_group) want[n_want++] = {sp.group_col_id, &ps->g};
  if (sp.has_filter) want[n_want++] = {sp.filter_col_id, &ps->f};
  if (sp.filter2_on) want[n_want++] = {sp.filter2_col_id, &ps->f2};
  for (int a = 0; a < sp.n_aggs; a++)
    if (sp.aggs[a].kind != DAGG_COUNT_ROWS)
      want[n_want++] = {sp.aggs[a].col_id, &ps->a[a]};
  if (dev.d_celldir)
    for (int i = 0; i < n_want; i++)
      if (want[i].col < 1 || want[i].col > 16) return false;
  for (int i = 0; i < n_want; i++) {
    const DevRegion::ColPlane *p = dev_colplane_get(
        dev, want[i].col, budget, eng->stream, &eng->plane_builds);
    if (!p) return false;
    /* k_plane_agg / k_plane_fc take a decimal row for a ROWPARSE row, so a
       mostly-decimal plane is as useless to them as a tombstoned one */
    const uint64_t n_rp = hash ? p->n_rowparse : p->n_rowparse + p->n_dec;
    if (!hash && n_rp * 8 > dev.n_kv) return false;
    want[i].ref->val = p->val;
    want[i].ref->st = p->st;
    want[i].ref->n_rowparse = n_rp;
    want[i].ref->dir =
        dev.d_celldir ? dev.d_celldir + (uint64_t)(want[i].col - 1) * dev.n_kv
                      : nullptr;
  }
  if (hash) {
    /* a column referenced twice is loaded once (cfg3 groups by and averages
       the same column) */
    for (int a = 0; a < sp.n_aggs; a++) {
      const PlaneRef &r = ps->a[a];
      if (!r.val) continue;
      if (ps->g.val && r.val == ps->g.val) ps->a_src[a] = 1;
      else if (r.val == ps->f.val) ps->a_src[a] = 2;
      else if (r.val == ps->f2.val) ps->a_src[a] = 3;
      else
        for (int b = 0; b < a; b++)
          if (ps->a[b].val == r.val) { ps->a_src[a] = 4 + b; break; }
    }
  }
  PlaneFcArgs fa;
  if (nu && !hash && !getenv("COPR_NO_NARROW") &&
      dev_plane_fc_shape(sp, *ps, &fa)) {
    const DevRegion::ColPlane *np = dev_colplane_narrow(
        dev, sp.filter_col_id, budget, eng->stream, &eng->narrow_builds);
    NarrowFcArgs nf;
    if (np && narrow_fc_fold(fa, np->nar_base, np->nar_nmax,
                             sp.filter_col_unsigned != 0, &nf)) {
      nu->p = np;
      nu->nf = nf;
      /* COPR_SPLIT_ALL_LO=1 (read per call): every row is resolved from both
         halves, the split kernel's worst case; same result bytes */
      if (np->nar_lo_off)
        split_fc_fold(nf, getenv("COPR_SPLIT_ALL_LO") != nullptr, &nu->sf);
    }
  }
  return true;
}


/* general selection translation: flatten the condition programs into one
   DevRpnNode program over <=4 distinct int columns, a gate node between
   one condition and the next. Falls back from the fixed cmp fast path;
   takes the node set orc_exec eval_rpn accepts for ints
   (expr_eval.rs:205,264). */
static copr_status translate_rpn(const CoprExecutor &ex, HostPlan *pl,
                                 ScanPlan *sp) {
  struct Slot { int64_t col_id; int off; };
  Slot slots[4];
  int n_slots = 0;
  int n = 0;
  int depth = 0;
  DevRpnNode prog[COPR_MAX_RPN];
  auto push = [&](const DevRpnNode &nd, int darg) -> bool {
    if (n >= COPR_MAX_RPN) return false;
    depth += darg;
    if (depth > 4 || depth < 1) return false;
    prog[n++] = nd;
    return true;
  };
  for (uint32_t c = 0; c < ex.n_conditions; c++) {
    const CoprExpr &cond = ex.conditions[c];
    if (c > 0) {
      /* a later condition sees only the rows the earlier ones kept
         (selection_executor.rs:86): the gate drops a row whose condition
         value is not true and empties the stack for the next condition */
      if (depth != 1) return COPR_ERR_INVALID_REQUEST;
      if (n >= COPR_MAX_RPN) return COPR_ERR_UNSUPPORTED;
      DevRpnNode gate{};
      gate.kind = 4;
      prog[n++] = gate;
      depth = 0;
    }
    for (uint32_t i = 0; i < cond.n_nodes; i++) {
      const CoprExprNode &en = cond.nodes[i];
      DevRpnNode nd{};
      switch (en.kind) {
        case COPR_EXPR_COLUMN_REF: {
          size_t off = (size_t)en.i64_val;
          if (off >= pl->cols.size()) return COPR_ERR_INVALID_REQUEST;
          const CoprColumnInfo &ci = pl->cols[off];
          if (!et_int(ci.ft.tp) || ci.pk_handle) return COPR_ERR_UNSUPPORTED;
          int s = -1;
          for (int t = 0; t < n_slots; t++)
            if (slots[t].col_id == ci.column_id) s = t;
          if (s < 0) {
            if (n_slots == 4) return COPR_ERR_UNSUPPORTED;
            slots[n_slots] = {ci.column_id, (int)off};
            s = n_slots++;
          }
          nd.kind = 0;
          nd.slot = s;
          nd.uns = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
          if (!push(nd, +1)) return COPR_ERR_UNSUPPORTED;
          break;
        }
        case COPR_EXPR_CONST_INT:
        case COPR_EXPR_CONST_UINT:
          nd.kind = 1;
          nd.cval = en.i64_val;
          nd.uns = en.kind == COPR_EXPR_CONST_UINT ? 1 : 0;
          if (!push(nd, +1)) return COPR_ERR_UNSUPPORTED;
          break;
        case COPR_EXPR_CONST_NULL:
          nd.kind = 2;
          if (!push(nd, +1)) return COPR_ERR_UNSUPPORTED;
          break;
        case COPR_EXPR_SCALAR_FUNC: {
          int na;
          switch (en.sig) {
            case COPR_SIG_LT_INT: case COPR_SIG_LE_INT: case COPR_SIG_GT_INT:
            case COPR_SIG_GE_INT: case COPR_SIG_EQ_INT: case COPR_SIG_NE_INT:
            case COPR_SIG_LOGICAL_AND: case COPR_SIG_LOGICAL_OR:
            case COPR_SIG_PLUS_INT: case COPR_SIG_MINUS_INT:
            case COPR_SIG_MULTIPLY_INT:
              na = 2;
              break;
            case COPR_SIG_UNARY_NOT: case COPR_SIG_INT_IS_NULL:
            case COPR_SIG_INT_IS_TRUE: case COPR_SIG_INT_IS_FALSE:
              na = 1;
              break;
            default:
              return COPR_ERR_UNSUPPORTED;
          }
          if (en.n_args != na) return COPR_ERR_INVALID_REQUEST;
          nd.kind = 3;
          nd.sig = en.sig;
          nd.uns = (en.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
          if (!push(nd, 1 - na)) return COPR_ERR_UNSUPPORTED;
          break;
        }
        default:
          return COPR_ERR_UNSUPPORTED;
      }
    }
  }
  if (depth != 1 || n == 0) return COPR_ERR_INVALID_REQUEST;
  /* capture channels + missing fill (scan default fill precedes the
     predicate, table_scan_executor.rs:456-483) */
  auto fill = [&](const CoprColumnInfo &ci, int32_t *mnull, int64_t *mval)
      -> copr_status {
    if (ci.default_val && ci.default_val_len) {
      int64_t dv;
      int r = host_decode_int_datum(ci.default_val, ci.default_val_len, &dv);
      if (r < 0) return COPR_ERR_INVALID_REQUEST;
      *mnull = r == 1 ? 1 : 0;
      *mval = dv;
    } else {
      *mnull = 1;
    }
    return COPR_OK;
  };
  if (n_slots >= 1) {
    const CoprColumnInfo &ci = pl->cols[slots[0].off];
    sp->has_filter = 1;
    sp->filter_col_id = ci.column_id;
    sp->filter_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    copr_status st = fill(ci, &sp->filter_missing_null,
                          &sp->filter_missing_val);
    if (st != COPR_OK) return st;
    pl->filter_col_offset = slots[0].off;
  }
  if (n_slots >= 2) {
    const CoprColumnInfo &ci = pl->cols[slots[1].off];
    sp->filter2_on = 1;
    sp->filter2_col_id = ci.column_id;
    sp->filter2_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    copr_status st = fill(ci, &sp->filter2_missing_null,
                          &sp->filter2_missing_val);
    if (st != COPR_OK) return st;
    pl->filter2_col_offset = slots[1].off;
  }
  /* channels 2..3: capture-only pseudo-agg slots (DAGG_XCAP). The agg
     node appends its own aggs AFTER the selection is planned, so reserve
     the TAIL slots; dev_idx for real aggs starts at 0 and xcap rides the
     high indices once n_aggs is final (patched in build_plan's agg pass:
     see xcap relocation below). Here we stage them at the front of
     sp->aggs beyond n_aggs=0 and record indices. */
  for (int k = 0; k + 2 < n_slots; k++) {
    const CoprColumnInfo &ci = pl->cols[slots[2 + k].off];
    DevAggSpec ds{};
    ds.kind = DAGG_XCAP;
    ds.col_id = ci.column_id;
    ds.col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    int idx = sp->n_aggs++;
    if (idx >= COPR_MAX_AGGS) return COPR_ERR_UNSUPPORTED;
    sp->aggs[idx] = ds;
    pl->xcap_col_offset[k] = slots[2 + k].off;
    sp->xcap_idx[sp->n_xcap] = idx;
    copr_status st = fill(ci, &sp->xcap_missing_null[sp->n_xcap],
                          &sp->xcap_missing_val[sp->n_xcap]);
    if (st != COPR_OK) return st;
    sp->n_xcap++;
  }
  sp->rpn_on = 1;
  sp->rpn_n = n;
  for (int i = 0; i < n; i++) sp->rpn[i] = prog[i];
  return COPR_OK;
}

static copr_status build_plan(const CoprDagRequest *req, HostPlan *pl) {
  if (req->n_executors == 0) return SET_ERR(COPR_ERR_INVALID_REQUEST, "empty executors");
  const CoprExecutor &scan = req->executors[0];
  if (scan.kind != COPR_EXEC_TABLE_SCAN && scan.kind != COPR_EXEC_INDEX_SCAN)
    return SET_ERR(COPR_ERR_UNSUPPORTED, "first executor must be a scan");
  pl->cols.assign(scan.columns, scan.columns + scan.n_columns);
  ScanPlan &sp = pl->sp;
  memset(&sp, 0, sizeof(sp));
  if (scan.kind == COPR_EXEC_INDEX_SCAN) {
    /* positional plan: rewrite each column's "id" to its datum position in
       the index key; the handle column sits at position n_idx_cols */
    sp.index_mode = 1;
    int pos = 0;
    for (auto &ci : pl->cols)
      if (!ci.pk_handle) {
        if (pos < COPR_MAX_OUT_COLS) sp.index_real_ids[pos] = ci.column_id;
        ci.column_id = pos++;
      }
    sp.index_n_cols = pos;
    for (auto &ci : pl->cols)
      if (ci.pk_handle) ci.column_id = pos;
  }

  const CoprExecutor *agg = nullptr;
  for (uint32_t e = 1; e < req->n_executors; e++) {
    const CoprExecutor &ex = req->executors[e];
    switch (ex.kind) {
      case COPR_EXEC_SELECTION: {
        /* conditions are ANDed (selection_executor.rs:86): up to two
           cmp(col, const) conjuncts take the fixed fast path; other int
           RPN shapes over <=2 distinct columns run through the device
           RPN evaluator */
        if (sp.has_filter || sp.rpn_on || ex.n_conditions < 1)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "one selection node supported");
        ScanPlan saved = sp;
        int saved_off = pl->filter_col_offset;
        copr_status st = ex.n_conditions <= 2
                             ? match_filter(ex.conditions[0], *pl, &sp)
                             : COPR_ERR_UNSUPPORTED;
        if (st != COPR_OK) {
          sp = saved;
          pl->filter_col_offset = saved_off;
          st = translate_rpn(ex, pl, &sp);
          if (st != COPR_OK)
            return SET_ERR(st, "unsupported selection condition shape");
          break;
        }
        if (ex.n_conditions == 2) {
          ScanPlan s2{};
          HostPlan p2;
          p2.cols = pl->cols;
          p2.sp.index_mode = sp.index_mode;
          st = match_filter(ex.conditions[1], p2, &s2);
          if (st != COPR_OK) {
            sp = saved;
            pl->filter_col_offset = saved_off;
            st = translate_rpn(ex, pl, &sp);
            if (st != COPR_OK)
              return SET_ERR(st, "unsupported selection condition shape");
            break;
          }
          sp.filter2_on = 1;
          sp.filter2_col_id = s2.filter_col_id;
          sp.filter2_is_real = s2.filter_is_real;
          sp.filter2_cmp = s2.filter_cmp;
          sp.filter2_const = s2.filter_const;
          sp.filter2_col_unsigned = s2.filter_col_unsigned;
          sp.filter2_const_unsigned = s2.filter_const_unsigned;
          sp.filter2_const_null = s2.filter_const_null;
          sp.filter2_missing_null = s2.filter_missing_null;
          sp.filter2_missing_val = s2.filter_missing_val;
          pl->filter2_col_offset = p2.filter_col_offset;
        }
        break;
      }
      case COPR_EXEC_SIMPLE_AGG: case COPR_EXEC_FAST_HASH_AGG:
      case COPR_EXEC_SLOW_HASH_AGG:
        /* SLOW_HASH_AGG plans as FAST_HASH_AGG does: the group-by list, not
           the executor kind, picks the path */
        if (agg) return SET_ERR(COPR_ERR_UNSUPPORTED, "one aggregation supported");
        agg = &ex;
        pl->hash_agg = ex.kind != COPR_EXEC_SIMPLE_AGG;
        break;
      case COPR_EXEC_STREAM_AGG:
        if (agg) return SET_ERR(COPR_ERR_UNSUPPORTED, "one aggregation supported");
        agg = &ex;
        pl->hash_agg = true;          /* same group-by plan shape */
        pl->stream_agg = true;
        break;
      case COPR_EXEC_TOPN: {
        if (pl->has_topn) return SET_ERR(COPR_ERR_UNSUPPORTED, "one TopN supported");
        if (ex.n_order_by == 0)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "one order-by expression supported");
        if (ex.n_order_by > 1) {
          /* several keys: each a COLUMN_REF to an int non-handle column of a
             table scan; a column that repeats cannot change the order after
             its first occurrence and is dropped */
          if (ex.n_order_by > COPR_TOPN_MAX_KEYS)
            return SET_ERR(COPR_ERR_UNSUPPORTED,
                           "multi-key TopN: at most 4 order-by expressions");
          if (sp.index_mode)
            return SET_ERR(COPR_ERR_UNSUPPORTED,
                           "multi-key TopN over an index scan not yet native");
          for (uint32_t k = 0; k < ex.n_order_by; k++) {
            const CoprExpr &ke = ex.order_by[k];
            if (ke.n_nodes != 1 || ke.nodes[0].kind != COPR_EXPR_COLUMN_REF)
              return SET_ERR(COPR_ERR_UNSUPPORTED,
                             "multi-key TopN: order-by must be a column");
            size_t koff = (size_t)ke.nodes[0].i64_val;
            if (koff >= pl->cols.size())
              return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad order-by offset");
            const CoprColumnInfo &kc = pl->cols[koff];
            if (kc.pk_handle)
              return SET_ERR(COPR_ERR_UNSUPPORTED,
                             "multi-key TopN: handle column as order key "
                             "not yet native");
            if (!et_int(kc.ft.tp))
              return SET_ERR(COPR_ERR_UNSUPPORTED,
                             "multi-key TopN: order-by type not yet native");
            bool repeat = false;
            for (const copr::TopnKey &pk : pl->topn_keys)
              repeat |= pk.col_off == (int32_t)koff;
            if (repeat) continue;
            copr::TopnKey tk{};
            tk.col_id = kc.column_id;
            tk.col_off = (int32_t)koff;
            tk.uns = (kc.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
            tk.desc = (ex.order_desc && ex.order_desc[k] != 0) ? 1 : 0;
            /* absent cell: the scan's default fill, else NULL */
            tk.missing_null = 1;
            if (kc.default_val && kc.default_val_len) {
              int64_t dv;
              int r = host_decode_int_datum(kc.default_val, kc.default_val_len, &dv);
              if (r < 0) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad default");
              tk.missing_null = r == 1 ? 1 : 0;
              tk.missing_val = dv;
            }
            pl->topn_keys.push_back(tk);
          }
          pl->has_topn = true;
          pl->topn_multi = true;
          pl->topn_off = pl->topn_keys[0].col_off;
          pl->topn_n = ex.limit;
          pl->topn_desc = pl->topn_keys[0].desc;
          /* the extract pass (keep flags) parses the group slot: key 0 */
          sp.group_col_id = pl->topn_keys[0].col_id;
          sp.group_col_unsigned = pl->topn_keys[0].uns;
          break;
        }
        const CoprExpr &oe = ex.order_by[0];
        if (oe.n_nodes != 1 || oe.nodes[0].kind != COPR_EXPR_COLUMN_REF)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "order-by must be a column");
        size_t off = (size_t)oe.nodes[0].i64_val;
        if (off >= pl->cols.size())
          return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad order-by offset");
        const CoprColumnInfo &ci = pl->cols[off];
        if (!et_int(ci.ft.tp) || ci.pk_handle)
          return SET_ERR(COPR_ERR_UNSUPPORTED, "order-by type not yet native");
        pl->has_topn = true;
        pl->topn_off = (int)off;
        pl->topn_n = ex.limit;
        pl->topn_desc = ex.order_desc ? (ex.order_desc[0] != 0) : 0;
        /* the extract pass reuses the group-col slot for the order column */
        sp.group_col_id = ci.column_id;
        sp.group_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
        break;
      }
      case COPR_EXEC_LIMIT:
        pl->limit = ex.limit;
        break;
      default:
        return SET_ERR(COPR_ERR_UNSUPPORTED, "unsupported executor kind");
    }
  }

  if (agg && pl->has_topn)
    return SET_ERR(COPR_ERR_UNSUPPORTED, "TopN with aggregation unsupported");
  if (pl->topn_multi && (sp.rpn_on || sp.n_xcap))
    return SET_ERR(COPR_ERR_UNSUPPORTED,
                   "multi-key TopN supports cmp(col,const) predicates only "
                   "(no RPN or capture-channel predicates)");
  if (!agg) {
    if (sp.index_mode && sp.rpn_on)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "index project supports cmp(col,const) predicates only");
    if (sp.n_xcap && !pl->has_topn)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "plain project supports predicates over <=2 distinct "
                     "columns (the project kernel has no capture slots)");
    sp.mode = 0;
    sp.n_out = (int32_t)pl->cols.size();
    if (sp.n_out > COPR_MAX_OUT_COLS)
      return SET_ERR(COPR_ERR_UNSUPPORTED, "too many scan columns");
    for (int i = 0; i < sp.n_out; i++) {
      sp.out_col_ids[i] = pl->cols[i].column_id;
      sp.out_is_handle[i] = pl->cols[i].pk_handle ? 1 : 0;
      pl->out_schema.push_back(pl->cols[i].ft);
    }
    return COPR_OK;
  }

  /* aggregation plan */
  pl->has_agg = true;
  if (pl->stream_agg && sp.index_mode)
    return SET_ERR(COPR_ERR_UNSUPPORTED,
                   "stream agg over index scan not yet native");
  sp.mode = pl->stream_agg ? 3 : (pl->hash_agg ? 2 : 1);
  if (agg->n_aggs == 0 || agg->n_aggs > COPR_MAX_AGGS)
    return SET_ERR(COPR_ERR_UNSUPPORTED, "agg count out of range");
  /* the selection pass may have staged capture-only XCAP slots; real aggs
     take the low dev indices, xcap relocates to the tail afterwards */
  DevAggSpec xcap_saved[2];
  int n_xcap_saved = sp.n_xcap;
  for (int k = 0; k < n_xcap_saved; k++)
    xcap_saved[k] = sp.aggs[sp.xcap_idx[k]];
  sp.n_aggs = 0;
  for (uint32_t a = 0; a < agg->n_aggs; a++) {
    const CoprAggDef &ad = agg->aggs[a];
    const CoprExpr &arg = ad.arg;
    DevAggSpec ds{};
    HostPlan::OutAgg oa{};
    oa.func = ad.func;
    oa.out_ft = ad.out_ft;
    oa.dev_idx = sp.n_aggs;
    /* arg must be a single column ref or a single const */
    if (arg.n_nodes != 1) return SET_ERR(COPR_ERR_UNSUPPORTED, "agg arg must be simple");
    const CoprExprNode &an = arg.nodes[0];
    bool is_const = an.kind == COPR_EXPR_CONST_INT || an.kind == COPR_EXPR_CONST_UINT;
    bool is_null_const = an.kind == COPR_EXPR_CONST_NULL;
    const CoprColumnInfo *ci = nullptr;
    if (an.kind == COPR_EXPR_COLUMN_REF) {
      size_t off = (size_t)an.i64_val;
      if (off >= pl->cols.size()) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad col offset");
      ci = &pl->cols[off];
      if (ci->pk_handle && !sp.index_mode)
        return SET_ERR(COPR_ERR_UNSUPPORTED, "agg over handle column not yet supported");
    }
    switch (ad.func) {
      case COPR_AGG_COUNT:
        if (is_const) ds.kind = DAGG_COUNT_ROWS;
        else if (is_null_const) ds.kind = DAGG_COUNT_ROWS | 0; /* count(NULL)=0 */
        else if (ci && (et_int(ci->ft.tp) || ci->ft.tp == COPR_TP_NEWDECIMAL ||
                        ci->ft.tp == COPR_TP_VARCHAR || ci->ft.tp == COPR_TP_STRING ||
                        ci->ft.tp == COPR_TP_VARSTRING || ci->ft.tp == COPR_TP_BLOB ||
                        ci->ft.tp == COPR_TP_DOUBLE))
          ds.kind = DAGG_COUNT_COL;
        else return SET_ERR(COPR_ERR_UNSUPPORTED, "count arg unsupported");
        if (is_null_const) {
          /* count(NULL) never increments: encode as COUNT_COL on a column id
             that never exists */
          ds.kind = DAGG_COUNT_COL;
          ds.col_id = INT64_MIN + 1;
        }
        oa.in_kind = DAGG_COUNT_ROWS;
        break;
      case COPR_AGG_SUM: case COPR_AGG_AVG:
        if (!ci) return SET_ERR(COPR_ERR_UNSUPPORTED, "sum/avg needs a column");
        if (et_int(ci->ft.tp)) {
          ds.kind = DAGG_SUM_INT;   /* exact int sum == Decimal rewrite sum */
        } else if (ci->ft.tp == COPR_TP_DOUBLE) {
          /* f64 sum: parallel order -> 1-ULP class (north_star budget) */
          ds.kind = DAGG_SUM_REAL;
        } else if (ci->ft.tp == COPR_TP_NEWDECIMAL) {
          ds.kind = DAGG_SUM_DEC;
          ds.target_frac = ci->ft.decimal >= 0 ? ci->ft.decimal : 0;
          if (ds.target_frac > 18)
            return SET_ERR(COPR_ERR_UNSUPPORTED, "decimal frac too large");
        } else {
          return SET_ERR(COPR_ERR_UNSUPPORTED, "sum/avg over non-int/decimal");
        }
        oa.in_kind = ds.kind;
        break;
      case COPR_AGG_MAX: case COPR_AGG_MIN:
        if (ci && ci->ft.tp == COPR_TP_DOUBLE) {
          ds.kind = ad.func == COPR_AGG_MAX ? DAGG_MAX_REAL : DAGG_MIN_REAL;
        } else if (ci && et_int(ci->ft.tp)) {
          ds.kind = ad.func == COPR_AGG_MAX ? DAGG_MAX_INT : DAGG_MIN_INT;
        } else {
          return SET_ERR(COPR_ERR_UNSUPPORTED,
                         "max/min native only over int/double");
        }
        oa.in_kind = ds.kind;
        break;
      case COPR_AGG_FIRST:
        if (!ci || (!et_int(ci->ft.tp) && ci->ft.tp != COPR_TP_DOUBLE))
          return SET_ERR(COPR_ERR_UNSUPPORTED,
                         "first native only over int/double");
        ds.kind = DAGG_FIRST;
        oa.in_kind = DAGG_FIRST;
        break;
      case COPR_AGG_BIT_AND: case COPR_AGG_BIT_OR: case COPR_AGG_BIT_XOR:
        if (!ci || !et_int(ci->ft.tp))
          return SET_ERR(COPR_ERR_UNSUPPORTED, "bit ops native only over int");
        ds.kind = ad.func == COPR_AGG_BIT_AND ? DAGG_BIT_AND
                  : ad.func == COPR_AGG_BIT_OR ? DAGG_BIT_OR : DAGG_BIT_XOR;
        oa.in_kind = ds.kind;
        break;
      default:
        return SET_ERR(COPR_ERR_UNSUPPORTED, "agg func not yet native");
    }
    if (ci) {
      ds.col_id = ci->column_id;
      ds.col_unsigned = (ci->ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    }
    sp.aggs[sp.n_aggs++] = ds;
    pl->out_aggs.push_back(oa);
    /* out schema: AVG adds the count column first (impl_avg.rs:52-60) */
    if (ad.func == COPR_AGG_AVG) {
      CoprFieldType cnt_ft{};
      cnt_ft.tp = COPR_TP_LONGLONG; cnt_ft.flag = COPR_FLAG_UNSIGNED;
      cnt_ft.flen = -1; cnt_ft.decimal = -1; cnt_ft.collate = 63;
      pl->out_schema.push_back(cnt_ft);
    }
    pl->out_schema.push_back(ad.out_ft);
  }
  /* relocate staged XCAP capture slots to the tail dev indices */
  for (int k = 0; k < n_xcap_saved; k++) {
    if (sp.n_aggs >= COPR_MAX_AGGS)
      return SET_ERR(COPR_ERR_UNSUPPORTED, "agg+predicate column budget");
    sp.xcap_idx[k] = sp.n_aggs;
    sp.aggs[sp.n_aggs++] = xcap_saved[k];
  }
  bool any_first = false;
  for (int a = 0; a < sp.n_aggs; a++)
    if (sp.aggs[a].kind == DAGG_FIRST) any_first = true;
  if (pl->hash_agg && agg->n_group_by > 1) {
    /* several keys: each a COLUMN_REF to an int non-handle column of a table
       scan; a column named twice is one key, emitted at each position */
    if (pl->stream_agg)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "multi-key group-by: stream agg takes one group-by expr");
    if (agg->n_group_by > COPR_GROUP_MAX_KEYS)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "multi-key group-by: at most 4 group-by expressions");
    if (sp.index_mode)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "multi-key group-by over an index scan not yet native");
    if (sp.rpn_on || sp.n_xcap)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "multi-key group-by supports cmp(col,const) predicates "
                     "only (no RPN or capture-channel predicates)");
    for (uint32_t k = 0; k < agg->n_group_by; k++) {
      const CoprExpr &ge = agg->group_by[k];
      if (ge.n_nodes != 1 || ge.nodes[0].kind != COPR_EXPR_COLUMN_REF)
        return SET_ERR(COPR_ERR_UNSUPPORTED,
                       "multi-key group-by: group-by must be a column");
      size_t goff = (size_t)ge.nodes[0].i64_val;
      if (goff >= pl->cols.size())
        return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad group offset");
      const CoprColumnInfo &gc = pl->cols[goff];
      if (gc.pk_handle)
        return SET_ERR(COPR_ERR_UNSUPPORTED,
                       "multi-key group-by: handle column as group key not "
                       "yet native");
      if (!et_int(gc.ft.tp))
        return SET_ERR(COPR_ERR_UNSUPPORTED,
                       "multi-key group-by: group-by type not yet native");
      pl->out_schema.push_back(gc.ft);
      int at = -1;
      for (size_t q = 0; q < pl->group_keys.size(); q++)
        if (pl->group_keys[q].col_off == (int32_t)goff) at = (int)q;
      if (at < 0) {
        copr::GroupKey gk{};
        gk.col_id = gc.column_id;
        gk.col_off = (int32_t)goff;
        gk.uns = (gc.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
        /* absent cell: the scan's default fill, else NULL */
        gk.missing_null = 1;
        if (gc.default_val && gc.default_val_len) {
          int64_t dv;
          int r = host_decode_int_datum(gc.default_val, gc.default_val_len, &dv);
          if (r < 0) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad default");
          gk.missing_null = r == 1 ? 1 : 0;
          gk.missing_val = dv;
        }
        at = (int)pl->group_keys.size();
        pl->group_keys.push_back(gk);
      }
      pl->group_pos.push_back(at);
    }
    pl->group_multi = true;
    /* stage 2 is keyed by the group id; the scan-path extract pass of the
       sorted route still parses a group slot, and gets key 0's column */
    sp.mode = 2;
    sp.group_col_id = pl->group_keys[0].col_id;
    sp.group_col_unsigned = pl->group_keys[0].uns;
  } else if (pl->hash_agg) {
    if (agg->n_group_by != 1)
      return SET_ERR(COPR_ERR_UNSUPPORTED, "exactly one group-by expr");
    const CoprExpr &ge = agg->group_by[0];
    if (ge.n_nodes != 1 || ge.nodes[0].kind != COPR_EXPR_COLUMN_REF)
      return SET_ERR(COPR_ERR_UNSUPPORTED, "group-by must be a column");
    size_t off = (size_t)ge.nodes[0].i64_val;
    if (off >= pl->cols.size()) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad group offset");
    const CoprColumnInfo &ci = pl->cols[off];
    bool grp_bytes = ci.ft.tp == COPR_TP_VARCHAR || ci.ft.tp == COPR_TP_STRING ||
                     ci.ft.tp == COPR_TP_VARSTRING || ci.ft.tp == COPR_TP_BLOB;
    if ((!et_int(ci.ft.tp) && !grp_bytes) || (ci.pk_handle && !sp.index_mode))
      return SET_ERR(COPR_ERR_UNSUPPORTED, "group-by type not yet native");
    if (grp_bytes) {
      /* SlowHashAggregationImpl: encoded-bytes group keys
         (slow_hash_aggr_executor.rs:220,285) */
      if (sp.index_mode)
        return SET_ERR(COPR_ERR_UNSUPPORTED, "bytes group over index scan");
      sp.mode = 4;
    }
    sp.group_col_id = ci.column_id;
    sp.group_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    pl->group_ft = ci.ft;
    pl->out_schema.push_back(ci.ft);
    if (any_first && sp.mode == 2) {
      /* the atomic hash table cannot order rows; route through the
         sorted-segmented pipeline (exact u64 key compare) */
      sp.mode = 3;
      pl->hash_sorted = true;
    }
  } else if (any_first) {
    if (sp.index_mode)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "FIRST over index scan not yet native");
    /* simple agg with FIRST reroutes through a single-run stream pass
       (group col that never matches -> one NULL-key run) */
    sp.mode = 3;
    sp.group_col_id = INT64_MIN + 1;
    sp.group_col_unsigned = 0;
    pl->simple_as_stream = true;
  }
  return COPR_OK;
}

/* tiling: pick rows_per_tile from the region's max row size so the staged
 * tile fits the LDS budget (Guideline: 256-thread blocks; <=64 KiB tile
 * keeps >=2 blocks/CU of occupancy on the 160 KiB LDS). */
static void pick_tiling(const DevRegion &rgn, ScanPlan *sp,
                        bool force_nopipe = false, uint32_t extra_lds = 0) {
  sp->use_pipe = 0;
  uint32_t per_row = (sp->index_mode ? rgn.max_key_bytes : rgn.max_row_bytes) + 1;

  if (!force_nopipe && !getenv("COPR_NO_PIPE")) {
    /* glds double-buffer pipeline: 2 x (offs slab + vals slab [+ dir
       slabs]), 1 KiB granular. >= 2 blocks/CU needs <= ~78 KiB.
       extra_lds (e.g. the hash pre-agg table) eats into the budget. */
    uint32_t nslabs = sp->n_dir_slabs ? (uint32_t)sp->n_dir_slabs
                                      : (sp->dir_plane ? 1u : 0u);
    uint32_t ds = nslabs * 1024u;
    uint32_t budget = 76 * 1024 + 2 * ds;
    budget = budget > extra_lds ? budget - extra_lds : 0;
    uint32_t rows = 1024;
    while (rows > 64) {
      uint32_t os = (((rows + 1) * 8) + 1023u) & ~1023u;
      uint32_t vs = ((rows * per_row + 31u) + 1023u) & ~1023u;
      if (2 * (os + vs + ds) <= budget) break;
      rows /= 2;
    }
    uint32_t os = (((rows + 1) * 8) + 1023u) & ~1023u;
    uint32_t vs = ((rows * per_row + 31u) + 1023u) & ~1023u;
    if (rows >= 64 && 2 * (os + vs + ds) <= 160 * 1024 - 2048) {
      sp->use_pipe = 1;
      sp->rows_per_tile = rows;
      sp->offs_slab = os;
      sp->vals_slab = vs;
      sp->dir_slab = ds;
      /* +16: the branchless varint window may read past the last staged
         byte of the second buffer */
      sp->lds_bytes = 2 * (os + vs + ds) + 16;
      return;
    }
  }
  sp->dir_slab = 0;

  uint32_t budget = 64 * 1024;          /* >=2 blocks/CU on 160 KiB LDS */
  uint32_t rows = 1024;                 /* up to 4 rows per lane per tile */
  while (rows > 64 && (uint64_t)rows * per_row + 96 > budget) rows /= 2;
  if ((uint64_t)rows * per_row + 96 > budget) {
    /* giant rows: single-row tiles with exact size */
    rows = 1;
  }
  sp->rows_per_tile = rows;
  uint64_t lds = (uint64_t)rows * per_row + 96;
  if (rows == 1) lds = (uint64_t)rgn.max_row_bytes + 96;
  sp->lds_bytes = (uint32_t)lds;
}

/* ---- datum response encoders (product side) ---- */
static void enc_cmp_u64(std::vector<uint8_t> *out, uint64_t v) {
  uint8_t b[8];
  for (int i = 7; i >= 0; i--) { b[i] = (uint8_t)v; v >>= 8; }
  out->insert(out->end(), b, b + 8);
}
static void enc_datum_int(std::vector<uint8_t> *out, int64_t v, bool uns) {
  out->push_back(uns ? 4 : 3);
  enc_cmp_u64(out, uns ? (uint64_t)v : ((uint64_t)v ^ 0x8000000000000000ull));
}
static void enc_datum_null(std::vector<uint8_t> *out) { out->push_back(0); }
static void enc_datum_real(std::vector<uint8_t> *out, uint64_t bits) {
  /* FLOAT datum: comparable f64 (convert.rs:16-22) */
  out->push_back(5);
  uint64_t u = (bits & 0x8000000000000000ull) ? ~bits
                                              : (bits | 0x8000000000000000ull);
  for (int i = 7; i >= 0; i--) out->push_back((uint8_t)(u >> (8 * i)));
}
static void enc_datum_dec_scaled(std::vector<uint8_t> *out, __int128 scaled, uint8_t frac) {
  prod::PDec d = prod::pdec_from_scaled_i128(scaled, frac);
  uint8_t prec, fr;
  prod::pdec_prec_and_frac(d, &prec, &fr);
  uint8_t tmp[48];
  size_t n = prod::pdec_encode(d, prec, fr, tmp);
  out->push_back(6);
  out->insert(out->end(), tmp, tmp + n);
}
/* wide sums: 256-bit scaled value (see atomic_add_i256). Returns false on
   word_buf overflow (reference Res::Overflow -> request error). */
static bool enc_datum_dec_scaled256(std::vector<uint8_t> *out,
                                    const uint64_t limbs[4], uint8_t frac) {
  bool ovf = false;
  prod::PDec d = prod::pdec_from_scaled_i256(limbs, frac, &ovf);
  if (ovf) return false;
  uint8_t prec, fr;
  prod::pdec_prec_and_frac(d, &prec, &fr);
  uint8_t tmp[48];
  size_t n = prod::pdec_encode(d, prec, fr, tmp);
  out->push_back(6);
  out->insert(out->end(), tmp, tmp + n);
  return true;
}

static inline __int128 i128_of(unsigned long long lo, unsigned long long hi) {
  return ((__int128)(long long)hi << 64) | (__int128)lo;
}

/* append one group's agg columns + optional group key, honouring
 * output_offsets over the out schema */
struct GroupRow {
  std::vector<std::pair<bool, std::string>> cells;  /* encoded datum per out col */
};

static void encode_agg_row(const HostPlan &pl, const SimpleAggAcc *accs,
                           bool has_group, bool group_null, int64_t group_key,
                           std::vector<std::vector<uint8_t>> *cols_out,
                           const unsigned long long *ext = nullptr,
                           bool *enc_err = nullptr) {
  size_t oc = 0;
  for (auto &oa : pl.out_aggs) {
    const SimpleAggAcc &ac = accs[oa.dev_idx];
    if (oa.func == COPR_AGG_COUNT) {
      bool uns = (pl.out_schema[oc].flag & COPR_FLAG_UNSIGNED) != 0;
      enc_datum_int(&(*cols_out)[oc], (int64_t)ac.cnt, uns);
      oc++;
    } else if (oa.func == COPR_AGG_FIRST) {
      /* first row's value, NULL included (impl_first.rs) */
      bool uns = (pl.out_schema[oc].flag & COPR_FLAG_UNSIGNED) != 0;
      if (ac.cnt == 0 || ac.sum_hi) enc_datum_null(&(*cols_out)[oc]);
      else if (pl.out_schema[oc].tp == COPR_TP_DOUBLE)
        enc_datum_real(&(*cols_out)[oc], ac.sum_lo);
      else enc_datum_int(&(*cols_out)[oc], (int64_t)ac.sum_lo, uns);
      oc++;
    } else if (oa.func == COPR_AGG_MAX || oa.func == COPR_AGG_MIN) {
      /* undo the fold transform (d_fold_xform): MIN folded max over ~x */
      bool uns = (pl.out_schema[oc].flag & COPR_FLAG_UNSIGNED) != 0;
      if (ac.cnt == 0) enc_datum_null(&(*cols_out)[oc]);
      else if (oa.in_kind == DAGG_MAX_REAL || oa.in_kind == DAGG_MIN_REAL) {
        unsigned long long b = ac.sum_lo;
        if (oa.func == COPR_AGG_MIN) b = ~b;
        uint64_t bits = (b & 0x8000000000000000ull)
                            ? (b & 0x7FFFFFFFFFFFFFFFull)
                            : ~b;
        enc_datum_real(&(*cols_out)[oc], bits);
      } else {
        unsigned long long b = ac.sum_lo;
        if (oa.func == COPR_AGG_MIN) b = ~b;
        bool col_uns = pl.sp.aggs[oa.dev_idx].col_unsigned != 0;
        if (!col_uns) b ^= 0x8000000000000000ull;
        enc_datum_int(&(*cols_out)[oc], (int64_t)b, uns);
      }
      oc++;
    } else if (oa.func == COPR_AGG_BIT_AND || oa.func == COPR_AGG_BIT_OR ||
               oa.func == COPR_AGG_BIT_XOR) {
      bool uns = (pl.out_schema[oc].flag & COPR_FLAG_UNSIGNED) != 0;
      unsigned long long b = ac.sum_lo;
      if (oa.func == COPR_AGG_BIT_AND) b = ~b;   /* OR of complements */
      enc_datum_int(&(*cols_out)[oc], (int64_t)b, uns);
      oc++;
    } else {
      if (oa.func == COPR_AGG_AVG) {
        enc_datum_int(&(*cols_out)[oc], (int64_t)ac.cnt, true);
        oc++;
      }
      std::vector<uint8_t> &sumcol = (*cols_out)[oc++];
      if (ac.cnt == 0) { enc_datum_null(&sumcol); }
      else if (oa.in_kind == DAGG_SUM_REAL) {
        enc_datum_real(&sumcol, ac.sum_lo);   /* f64 bits live in sum_lo */
      } else {
        __int128 s = i128_of(ac.sum_lo, ac.sum_hi);
        uint8_t frac = oa.in_kind == DAGG_SUM_DEC
                           ? (uint8_t)pl.sp.aggs[oa.dev_idx].target_frac : 0;
        uint64_t sgn = s < 0 ? ~0ull : 0ull;
        if (ext && (ext[oa.dev_idx * 2] != sgn || ext[oa.dev_idx * 2 + 1] != sgn)) {
          /* the sum spilled past i128: encode the 256-bit value */
          uint64_t limbs[4] = {ac.sum_lo, ac.sum_hi, ext[oa.dev_idx * 2],
                               ext[oa.dev_idx * 2 + 1]};
          if (!enc_datum_dec_scaled256(&sumcol, limbs, frac) && enc_err)
            *enc_err = true;
        } else {
          enc_datum_dec_scaled(&sumcol, s, frac);
        }
      }
    }
  }
  if (has_group) {
    std::vector<uint8_t> &gcol = (*cols_out)[oc];
    if (group_null) enc_datum_null(&gcol);
    else enc_datum_int(&gcol, group_key, (pl.group_ft.flag & COPR_FLAG_UNSIGNED) != 0);
  }
}

}  // namespace



/* row-v2 raw cell -> v1 datum re-encode (compat_v1.rs:28-126): the
   engine-side restatement used when project outputs come from v2 rows */
static bool e_v2_cell_to_datum(int32_t tp, uint32_t ft_flag,
                               const uint8_t *cell, size_t n,
                               std::vector<uint8_t> *out) {
  auto le_u64 = [&](uint64_t *u) {
    if (n != 1 && n != 2 && n != 4 && n != 8) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < n; i++) v |= (uint64_t)cell[i] << (8 * i);
    *u = v;
    return true;
  };
  auto le_i64 = [&](int64_t *iv) {
    uint64_t v;
    if (!le_u64(&v)) return false;
    switch (n) {
      case 1: *iv = (int8_t)v; break;
      case 2: *iv = (int16_t)v; break;
      case 4: *iv = (int32_t)v; break;
      default: *iv = (int64_t)v; break;
    }
    return true;
  };
  auto be8 = [&](uint64_t u) {
    for (int i = 7; i >= 0; i--) out->push_back((uint8_t)(u >> (8 * i)));
  };
  switch (tp) {
    case COPR_TP_TINY: case COPR_TP_SHORT: case COPR_TP_INT24:
    case COPR_TP_LONG: case COPR_TP_LONGLONG: {
      if (ft_flag & COPR_FLAG_UNSIGNED) {
        uint64_t u;
        if (!le_u64(&u)) return false;
        out->push_back(4);
        be8(u);
      } else {
        int64_t iv;
        if (!le_i64(&iv)) return false;
        out->push_back(3);
        be8((uint64_t)iv ^ 0x8000000000000000ull);
      }
      return true;
    }
    case COPR_TP_FLOAT: case COPR_TP_DOUBLE:
      out->push_back(5);
      out->insert(out->end(), cell, cell + n);
      return true;
    case COPR_TP_VARCHAR: case COPR_TP_VARSTRING: case COPR_TP_STRING:
    case COPR_TP_BLOB: {
      out->push_back(2);
      uint64_t uv = (uint64_t)n << 1;
      while (uv >= 0x80) { out->push_back((uint8_t)(uv | 0x80)); uv >>= 7; }
      out->push_back((uint8_t)uv);
      out->insert(out->end(), cell, cell + n);
      return true;
    }
    case COPR_TP_NEWDECIMAL:
      out->push_back(6);
      out->insert(out->end(), cell, cell + n);
      return true;
    case COPR_TP_DURATION: {
      int64_t iv;
      if (!le_i64(&iv)) return false;
      out->push_back(7);
      be8((uint64_t)iv ^ 0x8000000000000000ull);
      return true;
    }
    case COPR_TP_DATE: case COPR_TP_DATETIME: case COPR_TP_TIMESTAMP: {
      uint64_t u;
      if (!le_u64(&u)) return false;
      out->push_back(4);
      be8(u);
      return true;
    }
    case COPR_TP_NULL:
      out->push_back(0);
      return true;
    default:
      return false;
  }
}

/* ---------------- TypeChunk response encoding (engine side) ----------------
 * chunk/column.rs:41-71,1052-1071; decimal.rs:2135-2142; one chunk per
 * executor batch (runner.rs:1188-1225). Independent product restatement of
 * the same wire format the oracle pins. */
namespace {

struct EChunkCol {
  bool fixed = true;
  uint32_t flen = 8;
  uint32_t length = 0, null_cnt = 0;
  std::vector<uint8_t> bitmap, data;
  std::vector<int64_t> offsets{0};
  bool init(const CoprFieldType &ft) {
    switch (ft.tp) {
      case COPR_TP_TINY: case COPR_TP_SHORT: case COPR_TP_INT24:
      case COPR_TP_LONG: case COPR_TP_LONGLONG: case COPR_TP_YEAR:
      case COPR_TP_DOUBLE: case COPR_TP_DURATION:
        fixed = true; flen = 8; return true;
      case COPR_TP_NEWDECIMAL:
        fixed = true; flen = 40; return true;
      case COPR_TP_VARCHAR: case COPR_TP_STRING: case COPR_TP_VARSTRING:
      case COPR_TP_BLOB:
        fixed = false; return true;
      default:
        return false;
    }
  }
  void bit(bool notnull) {
    if ((length & 7) == 0) bitmap.push_back(0);
    if (notnull) bitmap[length >> 3] |= (uint8_t)(1u << (length & 7));
    else null_cnt++;
  }
  void app_null() {
    bit(false);
    if (fixed) data.insert(data.end(), flen, 0);
    else offsets.push_back(offsets.back());
    length++;
  }
  void app_fixed(const uint8_t *p, uint32_t n) {
    bit(true);
    data.insert(data.end(), p, p + n);
    if (n < flen) data.insert(data.end(), flen - n, 0);
    length++;
  }
  void app_var(const uint8_t *p, size_t n) {
    bit(true);
    data.insert(data.end(), p, p + n);
    offsets.push_back(offsets.back() + (int64_t)n);
    length++;
  }
  void flush(std::vector<uint8_t> *out) {
    uint8_t w[8];
    auto u32le = [&](uint32_t v) {
      w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8);
      w[2] = (uint8_t)(v >> 16); w[3] = (uint8_t)(v >> 24);
      out->insert(out->end(), w, w + 4);
    };
    u32le(length);
    u32le(null_cnt);
    if (null_cnt > 0) out->insert(out->end(), bitmap.begin(), bitmap.end());
    if (!fixed) {
      for (int64_t v : offsets) {
        uint64_t u = (uint64_t)v;
        for (int i = 0; i < 8; i++) w[i] = (uint8_t)(u >> (8 * i));
        out->insert(out->end(), w, w + 8);
      }
    }
    out->insert(out->end(), data.begin(), data.end());
  }
};

static bool e_var_u64(const uint8_t *p, size_t rem, uint64_t *v, size_t *n) {
  uint64_t uv = 0;
  size_t i = 0;
  int sh = 0;
  while (i < rem && i < 10) {
    uint8_t b = p[i++];
    uv |= (uint64_t)(b & 0x7F) << sh;
    sh += 7;
    if (!(b & 0x80)) { *v = uv; *n = i; return true; }
  }
  return false;
}

static size_t e_chunk_append_datum(EChunkCol *c, const uint8_t *p,
                                   size_t rem) {
  if (!rem) return 0;
  uint8_t flag = p[0];
  uint8_t tmp[8];
  switch (flag) {
    case 0:
      c->app_null();
      return 1;
    case 3: case 4: {
      if (rem < 9) return 0;
      uint64_t u = 0;
      for (int i = 0; i < 8; i++) u = (u << 8) | p[1 + i];
      if (flag == 3) u ^= 0x8000000000000000ull;
      for (int i = 0; i < 8; i++) tmp[i] = (uint8_t)(u >> (8 * i));
      c->app_fixed(tmp, 8);
      return 9;
    }
    case 5: {
      if (rem < 9) return 0;
      uint64_t u = 0;
      for (int i = 0; i < 8; i++) u = (u << 8) | p[1 + i];
      if (u & 0x8000000000000000ull) u &= 0x7FFFFFFFFFFFFFFFull;
      else u = ~u;
      for (int i = 0; i < 8; i++) tmp[i] = (uint8_t)(u >> (8 * i));
      c->app_fixed(tmp, 8);
      return 9;
    }
    case 8: case 9: {
      uint64_t uv;
      size_t n;
      if (!e_var_u64(p + 1, rem - 1, &uv, &n)) return 0;
      uint64_t u = uv;
      if (flag == 8) {
        uint64_t half = uv >> 1;
        u = (uv & 1) ? ~half : half;
      }
      for (int i = 0; i < 8; i++) tmp[i] = (uint8_t)(u >> (8 * i));
      c->app_fixed(tmp, 8);
      return 1 + n;
    }
    case 6: {
      prod::PDec d;
      uint8_t rf = 0;
      size_t used = 0;
      if (!prod::pdec_decode(p + 1, rem - 1, &d, &rf, &used)) return 0;
      uint8_t buf[40];
      buf[0] = d.int_cnt; buf[1] = d.frac_cnt; buf[2] = rf;
      buf[3] = d.negative ? 1 : 0;
      for (int i = 0; i < 9; i++) {
        uint32_t w = d.word_buf[i];
        buf[4 + 4 * i] = (uint8_t)w;
        buf[5 + 4 * i] = (uint8_t)(w >> 8);
        buf[6 + 4 * i] = (uint8_t)(w >> 16);
        buf[7 + 4 * i] = (uint8_t)(w >> 24);
      }
      c->app_fixed(buf, 40);
      return 1 + used;
    }
    case 2: {
      uint64_t uv;
      size_t nb;
      if (!e_var_u64(p + 1, rem - 1, &uv, &nb)) return 0;
      int64_t n = (uv & 1) ? (int64_t)(~(uv >> 1)) : (int64_t)(uv >> 1);
      if (n < 0 || 1 + nb + (uint64_t)n > rem) return 0;
      c->app_var(p + 1 + nb, (size_t)n);
      return 1 + nb + (size_t)n;
    }
    default:
      return 0;   /* memcomparable bytes not produced by these paths */
  }
}

static bool e_chunk_encode_post(const std::vector<uint8_t> &datum_resp,
                                const std::vector<uint64_t> &rows_per_chunk,
                                const std::vector<CoprFieldType> &out_fts,
                                std::vector<uint8_t> *out) {
  size_t p = 0;
  size_t nc = out_fts.size();
  for (uint64_t nrows : rows_per_chunk) {
    if (!nrows) continue;
    std::vector<EChunkCol> cols(nc);
    for (size_t c = 0; c < nc; c++)
      if (!cols[c].init(out_fts[c])) return false;
    for (uint64_t r = 0; r < nrows; r++) {
      for (size_t c = 0; c < nc; c++) {
        size_t used = e_chunk_append_datum(&cols[c], datum_resp.data() + p,
                                           datum_resp.size() - p);
        if (!used) return false;
        p += used;
      }
    }
    for (size_t c = 0; c < nc; c++) cols[c].flush(out);
  }
  return p == datum_resp.size();
}

}  // namespace

/* ---------------- DAG run ---------------- */
extern "C" copr_status copr_dag_run(copr_engine *eng, const CoprDagRequest *req,
                                    copr_region *const *regions, uint32_t n_regions,
                                    CoprSelectResult *out) {
  memset(out, 0, sizeof(*out));
  out->resume_row = UINT64_MAX;
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  if (req->paging_size && n_regions > 1)
    return SET_ERR(COPR_ERR_UNSUPPORTED,
                   "paging_size supports one region per request (the "
                   "reference pages per coprocessor task = per Region)");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  HostPlan pl;
  copr_status st = build_plan(req, &pl);
  if (st != COPR_OK) return st;

  if (eng->dec_col_off >= 0 && !pl.has_agg && !pl.has_topn &&
      !pl.sp.has_filter && (size_t)eng->dec_col_off < pl.cols.size()) {
    /* TopN sub-region project: the order column was decoded in place by
       the order expression -> output it in decoded form */
    const CoprColumnInfo &ci = pl.cols[eng->dec_col_off];
    pl.filter_col_offset = eng->dec_col_off;
    pl.sp.has_filter = 1;
    pl.sp.filter_decode_only = 1;
    pl.sp.filter_col_id = ci.column_id;
    pl.sp.filter_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    if (ci.default_val && ci.default_val_len) {
      int64_t dv;
      int r = host_decode_int_datum(ci.default_val, ci.default_val_len, &dv);
      if (r < 0) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad default");
      pl.sp.filter_missing_null = r == 1 ? 1 : 0;
      pl.sp.filter_missing_val = dv;
    } else {
      pl.sp.filter_missing_null = 1;
    }
  }
  if (pl.sp.filter2_on && pl.sp.mode == 0 && !pl.has_topn &&
      pl.filter2_col_offset >= 0) {
    /* expression-decoded output for the second predicate column */
    const CoprColumnInfo &ci = pl.cols[pl.filter2_col_offset];
    pl.dec2_col_offset = pl.filter2_col_offset;
    pl.sp.dec2_col_id = ci.column_id;
    pl.sp.dec2_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    pl.sp.dec2_missing_null = pl.sp.filter2_missing_null;
    pl.sp.dec2_missing_val = pl.sp.filter2_missing_val;
  }
  if (eng->dec2_col_off >= 0 && !pl.has_agg && !pl.has_topn &&
      (size_t)eng->dec2_col_off < pl.cols.size() &&
      eng->dec2_col_off != eng->dec_col_off) {
    const CoprColumnInfo &ci = pl.cols[eng->dec2_col_off];
    pl.dec2_col_offset = eng->dec2_col_off;
    pl.sp.dec2_col_id = ci.column_id;
    pl.sp.dec2_col_unsigned = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
    if (ci.default_val && ci.default_val_len) {
      int64_t dv;
      int r = host_decode_int_datum(ci.default_val, ci.default_val_len, &dv);
      if (r < 0) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad default");
      pl.sp.dec2_missing_null = r == 1 ? 1 : 0;
      pl.sp.dec2_missing_val = dv;
    } else {
      pl.sp.dec2_missing_null = 1;
    }
  }

  std::vector<uint8_t> resp;
  uint64_t n_rows_out = 0;
  /* TypeChunk segmentation (one chunk per executor batch; drains in
     1024-row chunks) */
  std::vector<uint64_t> chunk_rows;
  /* the device chunk encoder produced the final TypeChunk bytes directly */
  bool dev_chunked = false;
  /* HIP-event timing of the scan kernel(s), on the engine's own stream —
     reported in summaries[0].time_processed_ns (the ExecSummary surface the
     reference fills per executor slot, execute_stats.rs:43-76). bench.py's
     roofline leg reads this. */
  struct EventPair {             /* RAII: every error return destroys both */
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() { hipEventCreate(&a); hipEventCreate(&b); }
    ~EventPair() {
      if (a) hipEventDestroy(a);
      if (b) hipEventDestroy(b);
    }
  } ev;
  hipEvent_t ev_a = ev.a, ev_b = ev.b;
  float kernel_ms = 0.0f;
  bool timed = false;

  if (pl.has_topn) {
    /* ---- TopN: winner selection on device, then the regular project path
       over a gathered sub-region (rows already in output order) ---- */
    if (n_regions != 1)
      return SET_ERR(COPR_ERR_UNSUPPORTED, "TopN supports one region per request");
    copr_region *r = regions[0];
    ScanPlan sp = pl.sp;
    wire_celldir(&sp, r->dev);
    pick_tiling(r->dev, &sp, /*force_nopipe=*/true);
    uint64_t take_n = pl.topn_n < pl.limit ? pl.topn_n : pl.limit;
    std::vector<uint32_t> winners;
    /* multi-key: the winners' decoded key values, one list per key */
    std::vector<int64_t> key_vals[COPR_TOPN_MAX_KEYS];
    std::vector<uint8_t> key_nulls[COPR_TOPN_MAX_KEYS];
    int rc;
    if (pl.topn_multi) {
      uint64_t kept = 0, cands = 0;
      rc = dev_topn_multi_select(sp, r->dev, take_n, pl.topn_keys.data(),
                                 (int)pl.topn_keys.size(), eng->stream,
                                 &winners, key_vals, key_nulls, &kept, &cands);
      if (rc == 0) {
        eng->topn_multi_runs++;
        eng->topn_last_kept = kept;
        eng->topn_last_candidates = cands;
      }
    } else {
      rc = dev_topn_select(sp, r->dev, take_n, pl.topn_desc, eng->stream,
                           &winners);
    }
    if (rc == -3) return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
    if (rc == -2) return SET_ERR(COPR_ERR_OOM, "topn temp alloc");
    if (rc) return SET_ERR(COPR_ERR_INTERNAL, "topn selection failed");
    if (winners.empty()) {
      out->data = (uint8_t *)malloc(1);
      out->data_len = 0;
      out->n_rows = 0;
      out->summaries = (CoprExecSummary *)calloc(req->n_executors,
                                                 sizeof(CoprExecSummary));
      out->n_summaries = req->n_executors;
      return COPR_OK;
    }
    DevRegion sub{};
    rc = dev_subregion_build(r->dev, winners.data(), winners.size(), &sub,
                             eng->stream);
    if (rc)
      return SET_ERR(rc == -2 ? COPR_ERR_OOM : COPR_ERR_INTERNAL,
                     "subregion build failed");
    copr_region tmp;
    tmp.eng = eng;
    tmp.dev = sub;
    auto free_sub = [&]() {
      hipFree(sub.d_keys); hipFree(sub.d_key_offs);
      hipFree(sub.d_vals); hipFree(sub.d_val_offs);
      if (sub.d_celldir) hipFree(sub.d_celldir);
    };
    tmp.h_key_offs.resize(sub.n_kv + 1);
    tmp.h_val_offs.resize(sub.n_kv + 1);
    hipError_t ce = hipMemcpy(tmp.h_key_offs.data(), sub.d_key_offs,
                              (sub.n_kv + 1) * 8, hipMemcpyDeviceToHost);
    if (ce == hipSuccess)
      ce = hipMemcpy(tmp.h_val_offs.data(), sub.d_val_offs, (sub.n_kv + 1) * 8,
                     hipMemcpyDeviceToHost);
    if (ce != hipSuccess) {
      free_sub();
      return SET_ERR(COPR_ERR_INTERNAL, "subregion offs readback");
    }
    uint32_t mr = 0, mk = 0;
    for (uint64_t i = 0; i < sub.n_kv; i++) {
      uint64_t l = tmp.h_val_offs[i + 1] - tmp.h_val_offs[i];
      if (l > mr) mr = (uint32_t)l;
      uint64_t kl = tmp.h_key_offs[i + 1] - tmp.h_key_offs[i];
      if (kl > mk) mk = (uint32_t)kl;
    }
    tmp.dev.max_row_bytes = mr;
    tmp.dev.max_key_bytes = mk;
    /* plain project request over the sub-region: the scan node + the
       original output offsets (paging not applicable -- <= n rows) */
    CoprExecutor scan_ex = req->executors[0];
    scan_ex.conditions = nullptr; scan_ex.n_conditions = 0;
    CoprDagRequest preq{};
    preq.executors = &scan_ex;
    preq.n_executors = 1;
    preq.output_offsets = req->output_offsets;
    preq.n_output_offsets = req->n_output_offsets;
    preq.flags = req->flags;
    preq.div_precision_increment = req->div_precision_increment;
    copr_region *rp = &tmp;
    preq.encode_type = 0;                 /* post-encode below if chunked */
    if (pl.topn_multi) {
      /* every order column is emitted decoded from the key values the
         selection already produced; the two decode slots stay free for the
         int predicate columns that are not order columns. A Real predicate
         column needs none: its decoded datum equals its raw one. */
      auto is_key = [&](int off) {
        for (const copr::TopnKey &k : pl.topn_keys)
          if (k.col_off == off) return true;
        return false;
      };
      int d1 = -1, d2 = -1;
      if (pl.sp.has_filter && !pl.sp.filter_is_real &&
          pl.filter_col_offset >= 0 && !is_key(pl.filter_col_offset))
        d1 = pl.filter_col_offset;
      if (pl.sp.filter2_on && !pl.sp.filter2_is_real &&
          pl.filter2_col_offset >= 0 && !is_key(pl.filter2_col_offset) &&
          pl.filter2_col_offset != d1) {
        if (d1 < 0) d1 = pl.filter2_col_offset;
        else d2 = pl.filter2_col_offset;
      }
      eng->dec_col_off = d1;
      eng->dec2_col_off = d2;
      eng->topn_dec.clear();
      for (size_t k = 0; k < pl.topn_keys.size(); k++) {
        copr_engine::DecOverride ov;
        ov.col_off = pl.topn_keys[k].col_off;
        ov.uns = pl.topn_keys[k].uns != 0;
        ov.vals = std::move(key_vals[k]);
        ov.nulls = std::move(key_nulls[k]);
        eng->topn_dec.push_back(std::move(ov));
      }
    } else {
      eng->dec_col_off = pl.topn_off;
      eng->dec2_col_off =
          (pl.sp.has_filter && pl.filter_col_offset >= 0 &&
           pl.filter_col_offset != pl.topn_off) ? pl.filter_col_offset : -1;
      /* the selection decoded every column it names: those beyond the two
         decode slots are decoded by the host assembly */
      const int more[3] = {pl.sp.filter2_on && !pl.sp.filter2_is_real
                               ? pl.filter2_col_offset : -1,
                           pl.xcap_col_offset[0], pl.xcap_col_offset[1]};
      for (int off : more)
        if (off >= 0 && off != pl.topn_off && off != eng->dec2_col_off)
          eng->host_dec_offs.push_back(off);
    }
    copr_status st2 = copr_dag_run(eng, &preq, &rp, 1, out);
    eng->dec_col_off = -1;
    eng->dec2_col_off = -1;
    eng->topn_dec.clear();
    eng->host_dec_offs.clear();
    free_sub();
    if (st2 == COPR_OK && req->encode_type == 1) {
      std::vector<uint8_t> dat(out->data, out->data + out->data_len);
      std::vector<uint64_t> chunks;
      for (uint64_t left = out->n_rows; left;) {
        uint64_t b = left < 1024 ? left : 1024;
        chunks.push_back(b);
        left -= b;
      }
      std::vector<CoprFieldType> fts;
      for (uint32_t oo = 0; oo < req->n_output_offsets; oo++)
        fts.push_back(pl.out_schema[req->output_offsets[oo]]);
      std::vector<uint8_t> chunked;
      if (!e_chunk_encode_post(dat, chunks, fts, &chunked))
        return SET_ERR(COPR_ERR_UNSUPPORTED, "TypeChunk encode failed");
      free(out->data);
      out->data = (uint8_t *)malloc(chunked.size() ? chunked.size() : 1);
      memcpy(out->data, chunked.data(), chunked.size());
      out->data_len = chunked.size();
    }
    return st2;
  }

  if (pl.sp.mode == 3) {
    /* ---- stream agg: contiguous-run grouping in input order ---- */
    if (n_regions != 1)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "stream agg supports one region per request");
    copr_region *r = regions[0];
    ScanPlan sp = pl.sp;
    wire_celldir(&sp, r->dev);
    pick_tiling(r->dev, &sp, /*force_nopipe=*/true);
    std::vector<SimpleAggAcc> h_accs;
    std::vector<long long> h_gk;
    std::vector<uint8_t> h_gs;
    hipEventRecord(ev_a, eng->stream);
    int n_seg = pl.hash_sorted
                    ? dev_int_sorted_agg(sp, r->dev, eng->stream, &h_accs,
                                         &h_gk, &h_gs)
                    : dev_stream_agg(sp, r->dev, eng->stream, &h_accs, &h_gk,
                                     &h_gs);
    hipEventRecord(ev_b, eng->stream);
    timed = true;
    if (n_seg == -3)
      return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
    if (n_seg == -2) return SET_ERR(COPR_ERR_OOM, "stream agg temp alloc");
    if (n_seg < 0) return SET_ERR(COPR_ERR_INTERNAL, "stream agg failed");
    size_t n_out_cols = pl.out_schema.size();
    if (pl.simple_as_stream && n_seg == 0) {
      /* empty input: the reference still emits the one aggregate row */
      h_accs.assign(sp.n_aggs, SimpleAggAcc{});
      h_gk.assign(1, 0);
      h_gs.assign(1, 1);
      n_seg = 1;
    }
    uint64_t take = (uint64_t)n_seg < pl.limit ? (uint64_t)n_seg : pl.limit;
    for (uint64_t g = 0; g < take; g++) {
      std::vector<std::vector<uint8_t>> cols(n_out_cols);
      encode_agg_row(pl, &h_accs[g * sp.n_aggs], !pl.simple_as_stream,
                     h_gs[g] == 1, h_gk[g], &cols);
      for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
        uint32_t off = req->output_offsets[oo];
        if (off < n_out_cols)
          resp.insert(resp.end(), cols[off].begin(), cols[off].end());
      }
      n_rows_out++;
    }
  } else if (pl.sp.mode == 4) {
    /* ---- bytes-key hash agg ---- */
    if (n_regions != 1)
      return SET_ERR(COPR_ERR_UNSUPPORTED,
                     "bytes hash agg supports one region per request");
    copr_region *r = regions[0];
    ScanPlan sp = pl.sp;
    wire_celldir(&sp, r->dev);
    pick_tiling(r->dev, &sp, /*force_nopipe=*/true);
    std::vector<SimpleAggAcc> h_accs;
    std::vector<uint64_t> h_kofs;
    std::vector<uint32_t> h_klen;
    std::vector<uint8_t> h_kst;
    hipEventRecord(ev_a, eng->stream);
    int n_seg = dev_bytes_agg(sp, r->dev, eng->stream, &h_accs, &h_kofs,
                              &h_klen, &h_kst);
    hipEventRecord(ev_b, eng->stream);
    timed = true;
    if (n_seg == -3)
      return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
    if (n_seg == -2) return SET_ERR(COPR_ERR_OOM, "bytes agg temp alloc");
    if (n_seg < 0) return SET_ERR(COPR_ERR_INTERNAL, "bytes agg failed");
    size_t n_out_cols = pl.out_schema.size();
    uint64_t take = (uint64_t)n_seg < pl.limit ? (uint64_t)n_seg : pl.limit;
    /* one bulk readback of the value stream beats per-group copies when the
       region is small or the group count is large */
    std::vector<uint8_t> all_vals;
    if (n_seg > 64 && r->dev.val_bytes <= (256ull << 20)) {
      all_vals.resize(r->dev.val_bytes);
      if (hipMemcpy(all_vals.data(), r->dev.d_vals, r->dev.val_bytes,
                    hipMemcpyDeviceToHost) != hipSuccess)
        return SET_ERR(COPR_ERR_INTERNAL, "vals readback");
    }
    std::vector<uint8_t> keybuf;
    for (uint64_t g = 0; g < take; g++) {
      std::vector<std::vector<uint8_t>> cols(n_out_cols);
      encode_agg_row(pl, &h_accs[g * sp.n_aggs], false, false, 0, &cols);
      std::vector<uint8_t> &gcol = cols[n_out_cols - 1];
      if (h_kst[g] == 1) {
        gcol.push_back(0);                       /* NIL */
      } else {
        /* COMPACT_BYTES datum of the group payload (datum_codec.rs:290-294) */
        gcol.push_back(2);
        uint64_t uv = ((uint64_t)h_klen[g]) << 1;   /* zigzag, non-negative */
        while (uv >= 0x80) { gcol.push_back((uint8_t)(uv | 0x80)); uv >>= 7; }
        gcol.push_back((uint8_t)uv);
        if (!all_vals.empty()) {
          gcol.insert(gcol.end(), all_vals.data() + h_kofs[g],
                      all_vals.data() + h_kofs[g] + h_klen[g]);
        } else {
          keybuf.resize(h_klen[g]);
          if (h_klen[g]) {
            hipError_t ce2 = hipMemcpy(keybuf.data(),
                                       r->dev.d_vals + h_kofs[g], h_klen[g],
                                       hipMemcpyDeviceToHost);
            if (ce2 != hipSuccess)
              return SET_ERR(COPR_ERR_INTERNAL, "group key readback");
          }
          gcol.insert(gcol.end(), keybuf.begin(), keybuf.end());
        }
      }
      for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
        uint32_t off = req->output_offsets[oo];
        if (off < n_out_cols)
          resp.insert(resp.end(), cols[off].begin(), cols[off].end());
      }
      n_rows_out++;
    }
  } else
  if (pl.sp.mode == 1 || pl.sp.mode == 2) {
    if (pl.sp.mode == 1) {
      /* ---- simple agg: one accumulator set across all regions ---- */
      /* the accumulators persist on the engine across requests (the
         per-request hipMalloc/hipFree pair was most of the ~58 us of host
         work per call) and re-zero with async memsets */
      if (!eng->d_simple_acc) {
        HIP_TRY(hipMalloc(&eng->d_simple_acc,
                          sizeof(SimpleAggAcc) * (COPR_MAX_AGGS + 1)), "acc alloc");
        if (hipMalloc(&eng->d_simple_ext, COPR_MAX_AGGS * 16) != hipSuccess) {
          hipFree(eng->d_simple_acc);
          eng->d_simple_acc = nullptr;
          eng->d_simple_ext = nullptr;
          return SET_ERR(COPR_ERR_OOM, "acc ext alloc");
        }
      }
      SimpleAggAcc *d_acc = eng->d_simple_acc;
      unsigned long long *d_ext = nullptr;
      bool any_dec = false;
      for (int a = 0; a < pl.sp.n_aggs; a++)
        if (pl.sp.aggs[a].kind == DAGG_SUM_DEC || pl.sp.aggs[a].kind == DAGG_SUM_INT)
          any_dec = true;
      /* column planes: decided per region; a missing plane, and the filter
         plane's narrow companion, is built here, before the timed events, so
         time_processed_ns stays the query */
      std::vector<PlaneSet> psets;
      std::vector<NarrowUse> nuse;
      if (!getenv("COPR_NO_PLANES") && plane_plan_ok(pl.sp)) {
        psets.resize(n_regions);
        nuse.resize(n_regions);
        for (uint32_t rg = 0; rg < n_regions; rg++)
          if (!plane_wire(eng, regions[rg]->dev, pl.sp, &psets[rg], false,
                          &nuse[rg])) {
            psets[rg] = PlaneSet{};
            nuse[rg] = NarrowUse{};
          }
      }
      uint32_t fcn_grid = 0;   /* diagnostic: cap k_plane_fcn / _fcs' grid */
      if (const char *g = getenv("COPR_NARROW_GRID"))
        fcn_grid = (uint32_t)strtoul(g, nullptr, 10);
      /* one-dispatch step: every region takes k_plane_fcn (or,
         on a split plane, k_plane_fcs), so
         the whole result is one count, which the last launch's last block
         hands to the pinned host word while it re-zeroes the device words.
         No memset and no copy in the steady state. */
      bool one_dispatch = n_regions > 0 && !nuse.empty() &&
                          !getenv("COPR_NARROW_NO_FINALIZE");
      for (uint32_t rg = 0; one_dispatch && rg < n_regions; rg++)
        if (!nuse[rg].p) one_dispatch = false;
      if (one_dispatch && !eng->d_fcn_state) {
        /* first use; on failure the request takes the usual sequence */
        void *d = nullptr, *h = nullptr;
        if (hipMalloc(&d, COPR_FCN_STATE_WORDS * 8) == hipSuccess &&
            hipHostMalloc(&h, sizeof(unsigned long long),
                          hipHostMallocDefault) == hipSuccess) {
          eng->d_fcn_state = (unsigned long long *)d;
          eng->h_fcn_out = (unsigned long long *)h;
          eng->fcn_dirty = true;          /* zeroed below */
        } else {
          (void)hipGetLastError();
          hipFree(d);
          one_dispatch = false;
        }
      }
      if (one_dispatch && eng->fcn_dirty) {
        if (hipMemsetAsync(eng->d_fcn_state, 0, COPR_FCN_STATE_WORDS * 8,
                           eng->stream) == hipSuccess) {
          eng->fcn_dirty = false;
        } else {
          (void)hipGetLastError();
          one_dispatch = false;
        }
      }
      SimpleAggAcc h_acc[COPR_MAX_AGGS + 1];
      unsigned long long h_ext[COPR_MAX_AGGS * 2] = {0};
      if (one_dispatch) {
        unsigned long long *d_cnt = eng->d_fcn_state;
        unsigned int *d_ticket = (unsigned int *)(
            eng->d_fcn_state + COPR_FCN_SLOTS * COPR_FCN_SLOT_STRIDE);
        hipEventRecord(ev_a, eng->stream);
        for (uint32_t rg = 0; rg < n_regions; rg++) {
          const bool last = rg + 1 == n_regions;
          int e = dev_plane_fcn_launch(*nuse[rg].p, nuse[rg].nf, nuse[rg].sf,
                                       regions[rg]->dev.n_kv, d_cnt,
                                       COPR_FCN_SLOTS,
                                       last ? d_ticket : nullptr,
                                       last ? eng->h_fcn_out : nullptr,
                                       fcn_grid, eng->stream);
          eng->plane_launches++;
          eng->narrow_launches++;
          if (nuse[rg].p->nar_lo_off) eng->split_launches++;
          if (e) {
            eng->fcn_dirty = true;
            return SET_ERR(COPR_ERR_INTERNAL, "narrow plane launch failed");
          }
        }
        hipEventRecord(ev_b, eng->stream);
        timed = true;
        hipError_t ce = hipStreamSynchronize(eng->stream);
        if (ce != hipSuccess) {
          eng->fcn_dirty = true;
          return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(ce));
        }
        memset(h_acc, 0, sizeof(h_acc));
        h_acc[0].cnt = *(volatile unsigned long long *)eng->h_fcn_out;
      } else {
        HIP_TRY(hipMemsetAsync(d_acc, 0,
                               sizeof(SimpleAggAcc) * (COPR_MAX_AGGS + 1),
                               eng->stream), "acc memset");
        if (any_dec) {
          d_ext = eng->d_simple_ext;
          HIP_TRY(hipMemsetAsync(d_ext, 0, COPR_MAX_AGGS * 16, eng->stream),
                  "acc ext memset");
        }
        hipEventRecord(ev_a, eng->stream);
        for (uint32_t rg = 0; rg < n_regions; rg++) {
          ScanPlan sp = pl.sp;
          sp.simple_ext = d_ext;
          wire_celldir(&sp, regions[rg]->dev);
          int e;
          if (!nuse.empty() && nuse[rg].p) {
            /* a narrow region beside regions that are not: same kernel, the
               count joins the other regions' in the usual accumulator */
            e = dev_plane_fcn_launch(*nuse[rg].p, nuse[rg].nf, nuse[rg].sf,
                                     regions[rg]->dev.n_kv, &d_acc[0].cnt, 1,
                                     nullptr, nullptr, fcn_grid, eng->stream);
            eng->plane_launches++;
            eng->narrow_launches++;
            if (nuse[rg].p->nar_lo_off) eng->split_launches++;
          } else if (!psets.empty() && plane_set_used(psets[rg])) {
            e = dev_plane_agg_launch(sp, psets[rg], regions[rg]->dev, d_acc,
                                     eng->stream);
            eng->plane_launches++;
          } else {
            pick_tiling(regions[rg]->dev, &sp);
            e = dev_scan_launch(sp, regions[rg]->dev, d_acc, nullptr, nullptr, eng->stream);
          }
          if (e) return SET_ERR(COPR_ERR_INTERNAL, "scan launch failed");
        }
        hipEventRecord(ev_b, eng->stream);
        timed = true;
        hipError_t ce = hipMemcpyAsync(h_acc, d_acc, sizeof(h_acc), hipMemcpyDeviceToHost,
                                       eng->stream);
        if (ce == hipSuccess && d_ext)
          ce = hipMemcpyAsync(h_ext, d_ext, COPR_MAX_AGGS * 16,
                              hipMemcpyDeviceToHost, eng->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(eng->stream);
        if (ce != hipSuccess) return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(ce));
      }
      if (h_acc[COPR_MAX_AGGS].cnt & 1)
        return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
      /* encode the single result row */
      size_t n_out_cols = pl.out_schema.size();
      std::vector<std::vector<uint8_t>> cols(n_out_cols);
      bool enc_err = false;
      encode_agg_row(pl, h_acc, false, false, 0, &cols,
                     any_dec ? h_ext : nullptr, &enc_err);
      if (enc_err)
        return SET_ERR(COPR_ERR_STORAGE, "decimal sum overflow (Res::Overflow)");
      for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
        uint32_t off = req->output_offsets[oo];
        if (off >= n_out_cols) return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad output offset");
        resp.insert(resp.end(), cols[off].begin(), cols[off].end());
      }
      n_rows_out = 1;
    } else {
      /* ---- hash agg ---- */
      /* start small and grow x16 on overflow: GB-scale tables cost more
         in per-call allocation and init than a retry pass saves (measured:
         pre-sizing by row count regressed low-cardinality workloads 16x).
         The device-side compaction keeps the readback proportional to
         n_groups when the table does grow. */
      uint32_t tsize = 1u << 16;
      bool any_dec = false;
      for (int a = 0; a < pl.sp.n_aggs; a++)
        if (pl.sp.aggs[a].kind == DAGG_SUM_DEC) any_dec = true;
      auto ht_cache_drop = [&]() {
        HashAggTable &c = eng->ht_cache;
        hipFree(c.keys); hipFree(c.accs); hipFree(c.reserved);
        hipFree(c.ext); hipFree(c.rsvd_ext);
        hipFree(c.rsvd_seen); hipFree(c.error); hipFree(c.n_groups);
        c = HashAggTable{};
        eng->ht_cache_tsize = 0;
      };
      /* column planes: decided per region, all or nothing; a
         missing plane is built here, before the first attempt's timed
         events, and retries after a table-full reuse the wiring. A region
         without planes scans into the same table. */
      std::vector<PlaneSet> psets;
      if (!pl.group_multi && !getenv("COPR_NO_PLANES") &&
          hash_plane_plan_ok(pl.sp)) {
        psets.resize(n_regions);
        for (uint32_t rg = 0; rg < n_regions; rg++)
          if (!plane_wire(eng, regions[rg]->dev, pl.sp, &psets[rg], true))
            psets[rg] = PlaneSet{};
      }
      /* ---- several group-by columns: stage 1 turns every
         row's key tuple into one exact group id; stage 2 is the single-key
         machinery keyed by that id: k_plane_hash with the id buffer as its
         group plane when the other columns wire to planes, the sorted
         pipeline otherwise ---- */
      GroupIds gm{};
      struct GmGuard {
        GroupIds *g;
        ~GmGuard() { dev_group_free(g); }
      } gm_guard{&gm};
      bool gm_sorted = false;
      /* rows for the groups named by slot index: aggregates first, then the
         group columns in request order */
      auto emit_multi = [&](const long long *slots, uint64_t n_groups,
                            const SimpleAggAcc *accs,
                            const unsigned long long *ext) -> copr_status {
        const uint64_t take = n_groups < pl.limit ? n_groups : pl.limit;
        std::vector<uint32_t> which(take);
        for (uint64_t i = 0; i < take; i++) which[i] = (uint32_t)slots[i];
        std::vector<int64_t> gv;
        std::vector<uint8_t> gn;
        int grc = dev_group_gather(gm, which.data(), take, eng->stream, &gv, &gn);
        if (grc == -2) return SET_ERR(COPR_ERR_OOM, "group key gather alloc");
        if (grc) return SET_ERR(COPR_ERR_INTERNAL, "group key gather failed");
        const size_t n_out_cols = pl.out_schema.size();
        const size_t g0 = n_out_cols - pl.group_pos.size();
        const int na = pl.sp.n_aggs;
        bool enc_err = false;
        for (uint64_t i = 0; i < take; i++) {
          std::vector<std::vector<uint8_t>> cols(n_out_cols);
          encode_agg_row(pl, accs + i * na, false, false, 0, &cols,
                         ext ? ext + i * na * 2 : nullptr, &enc_err);
          for (size_t j = 0; j < pl.group_pos.size(); j++) {
            const int k = pl.group_pos[j];
            if (gn[(size_t)k * take + i]) enc_datum_null(&cols[g0 + j]);
            else
              enc_datum_int(&cols[g0 + j], gv[(size_t)k * take + i],
                            pl.group_keys[k].uns != 0);
          }
          for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
            uint32_t off = req->output_offsets[oo];
            if (off < n_out_cols)
              resp.insert(resp.end(), cols[off].begin(), cols[off].end());
          }
          n_rows_out++;
        }
        if (enc_err)
          return SET_ERR(COPR_ERR_STORAGE,
                         "decimal sum overflow (Res::Overflow)");
        return COPR_OK;
      };
      if (pl.group_multi) {
        if (n_regions != 1)
          return SET_ERR(COPR_ERR_UNSUPPORTED,
                         "multi-key group-by supports one region per request");
        DevRegion &dev = regions[0]->dev;
        if (dev.n_kv >= 0xFFFFFFFFull)
          return SET_ERR(COPR_ERR_UNSUPPORTED,
                         "multi-key group-by: region of 2^32 - 1 rows or more");
        const int K = (int)pl.group_keys.size();
        const bool planes_on = !getenv("COPR_NO_PLANES");
        /* key planes, built here (before the timed events) under the hash
           consumer's budget; one with rows left to the row bytes or decimal
           rows is not a key source */
        PlaneRef kp[COPR_GROUP_MAX_KEYS] = {};
        if (planes_on && dev.n_kv) {
          uint64_t budget = dev.val_bytes;
          if (const char *e = getenv("COPR_PLANE_BUDGET_MB"))
            budget = (uint64_t)strtoull(e, nullptr, 10) << 20;
          for (int k = 0; k < K; k++) {
            const DevRegion::ColPlane *p = dev_colplane_get(
                dev, pl.group_keys[k].col_id, budget, eng->stream,
                &eng->plane_builds);
            if (p && !p->n_rowparse && !p->n_dec)
              kp[k] = PlaneRef{p->val, p->st, nullptr, 0};
          }
        }
        if (planes_on && hash_plane_plan_ok(pl.sp)) {
          psets.resize(1);
          if (!plane_wire(eng, dev, pl.sp, &psets[0], true, nullptr,
                          /*wire_group=*/false))
            psets.clear();
        }
        uint32_t gk_slots = 1u << 16;
        if (const char *e = getenv("COPR_GK_SLOTS")) {
          unsigned long long v = strtoull(e, nullptr, 10);
          if (v && v <= (1ull << 31) && !(v & (v - 1))) gk_slots = (uint32_t)v;
        }
        hipEventRecord(ev_a, eng->stream);
        int grc = dev_group_ids(dev, pl.group_keys.data(), K, kp, gk_slots,
                                eng->stream, &gm);
        eng->group_dict_grows += gm.grows;
        eng->group_row_source_runs += gm.row_source_runs;
        if (grc == -3)
          return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
        if (grc == -2) return SET_ERR(COPR_ERR_OOM, "group id alloc");
        if (grc) return SET_ERR(COPR_ERR_INTERNAL, "group id stage failed");
        eng->group_multi_runs++;
        eng->group_last_groups = gm.n_groups;
        if (!psets.empty())
          psets[0].g = PlaneRef{gm.gid_val, gm.gid_st, nullptr, 0};
        else
          gm_sorted = true;
      }
      if (gm_sorted) {
        copr_region *r = regions[0];
        ScanPlan sp = pl.sp;
        sp.mode = 3;
        wire_celldir(&sp, r->dev);
        pick_tiling(r->dev, &sp, /*force_nopipe=*/true);
        std::vector<SimpleAggAcc> h_accs;
        std::vector<long long> h_gk;
        std::vector<uint8_t> h_gs;
        int n_seg = dev_int_sorted_agg(sp, r->dev, eng->stream, &h_accs, &h_gk,
                                       &h_gs, gm.gid_val);
        hipEventRecord(ev_b, eng->stream);
        timed = true;
        if (n_seg == -3)
          return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
        if (n_seg == -2) return SET_ERR(COPR_ERR_OOM, "sorted agg temp alloc");
        if (n_seg < 0) return SET_ERR(COPR_ERR_INTERNAL, "sorted agg failed");
        copr_status est = emit_multi(h_gk.data(), (uint64_t)n_seg,
                                     h_accs.data(), nullptr);
        if (est != COPR_OK) return est;
      } else
      for (int attempt = 0; attempt < 4; attempt++) {
        /* the table buffers persist on the engine across requests: the
           per-request hipMalloc/hipFree set measured ~3 ms at cfg3 scale */
        if (eng->ht_cache_tsize != tsize ||
            eng->ht_cache_naggs != pl.sp.n_aggs ||
            eng->ht_cache_ext != any_dec || !eng->ht_cache.keys) {
          ht_cache_drop();
          HashAggTable c{};
          hipError_t e = hipSuccess;
          if (e == hipSuccess) e = hipMalloc((void **)&c.keys, (size_t)tsize * 8);
          if (e == hipSuccess) e = hipMalloc((void **)&c.accs, (size_t)tsize * pl.sp.n_aggs * sizeof(SimpleAggAcc));
          if (e == hipSuccess) e = hipMalloc((void **)&c.reserved, 2 * pl.sp.n_aggs * sizeof(SimpleAggAcc));
          if (e == hipSuccess && any_dec)
            e = hipMalloc((void **)&c.ext, (size_t)tsize * pl.sp.n_aggs * 16);
          if (e == hipSuccess && any_dec)
            e = hipMalloc((void **)&c.rsvd_ext, 2 * pl.sp.n_aggs * 16);
          if (e == hipSuccess) e = hipMalloc((void **)&c.rsvd_seen, 2 * 8);
          if (e == hipSuccess) e = hipMalloc((void **)&c.error, 8);
          if (e == hipSuccess) e = hipMalloc((void **)&c.n_groups, 8);
          if (e != hipSuccess) {
            eng->ht_cache = c;
            ht_cache_drop();
            return SET_ERR(COPR_ERR_OOM, "hash table alloc");
          }
          eng->ht_cache = c;
          eng->ht_cache_tsize = tsize;
          eng->ht_cache_naggs = pl.sp.n_aggs;
          eng->ht_cache_ext = any_dec;
        }
        HashAggTable ht = eng->ht_cache;
        auto free_ht = [&]() { ht_cache_drop(); };
        /* re-init for this request (async; EMPTY = INT64_MIN needs a fill
           kernel, the byte pattern is not memset-able) */
        {
          hipError_t e = hipSuccess;
          dev_fill_keys(ht.keys, tsize, eng->stream);
          e = hipGetLastError();
          if (e == hipSuccess) e = hipMemsetAsync(ht.accs, 0, (size_t)tsize * pl.sp.n_aggs * sizeof(SimpleAggAcc), eng->stream);
          if (e == hipSuccess && ht.ext)
            e = hipMemsetAsync(ht.ext, 0, (size_t)tsize * pl.sp.n_aggs * 16, eng->stream);
          if (e == hipSuccess && ht.rsvd_ext)
            e = hipMemsetAsync(ht.rsvd_ext, 0, 2 * pl.sp.n_aggs * 16, eng->stream);
          if (e == hipSuccess) e = hipMemsetAsync(ht.reserved, 0, 2 * pl.sp.n_aggs * sizeof(SimpleAggAcc), eng->stream);
          if (e == hipSuccess) e = hipMemsetAsync(ht.rsvd_seen, 0, 16, eng->stream);
          if (e == hipSuccess) e = hipMemsetAsync(ht.error, 0, 8, eng->stream);
          if (e == hipSuccess) e = hipMemsetAsync(ht.n_groups, 0, 8, eng->stream);
          if (e != hipSuccess) { free_ht(); return SET_ERR(COPR_ERR_INTERNAL, "ht init"); }
        }
        /* several keys: ev_a went before stage 1 */
        if (!pl.group_multi) hipEventRecord(ev_a, eng->stream);
        for (uint32_t rg = 0; rg < n_regions; rg++) {
          ScanPlan sp = pl.sp;
          sp.table_size = tsize;
          wire_celldir(&sp, regions[rg]->dev);
          bool any_real_sum = false;
          for (int a = 0; a < sp.n_aggs; a++)
            if (sp.aggs[a].kind == DAGG_SUM_REAL) any_real_sum = true;
          /* the LDS pre-agg table accumulates sums with integer atomics;
             f64-bit sums go straight to the global table's double atomics */
          uint32_t slots = any_real_sum ? 0u : 256u;  /* pow2: probe masks */
          uint32_t table_b =
              slots ? (16u + slots * (8 + (uint32_t)sp.n_aggs *
                                              (uint32_t)sizeof(SimpleAggAcc)))
                    : 0u;
          while (slots && table_b > 100u * 1024u) {
            slots /= 2;
            table_b = 16u + slots * (8 + (uint32_t)sp.n_aggs *
                                             (uint32_t)sizeof(SimpleAggAcc));
          }
          if (!psets.empty() && plane_set_used(psets[rg])) {
            /* no row staging: the LDS holds the pre-agg table alone */
            sp.lds_agg_slots = slots;
            sp.lds_agg_off = 0;
            sp.lds_bytes = slots ? table_b - 16u : 0u;
            int le = dev_plane_hash_launch(sp, psets[rg], regions[rg]->dev,
                                           ht, eng->stream);
            eng->hash_plane_launches++;
            if (le) { free_ht(); return SET_ERR(COPR_ERR_INTERNAL, "plane hash launch failed"); }
            continue;
          }
          /* hash mode prefers the glds-pipelined kernel (DMA-staged dir
             planes + overlap; r01's single-buffer kernel measured 47%
             wave-parked); the table rides after the two buffers */
          pick_tiling(regions[rg]->dev, &sp, /*force_nopipe=*/false, table_b);
          if (!sp.use_pipe && sp.lds_bytes + table_b > 70 * 1024) {
            /* shrink the tile so table + tile keep >=2 blocks/CU */
            uint32_t per_row = regions[rg]->dev.max_row_bytes + 1;
            uint32_t rows = sp.rows_per_tile;
            while (rows > 64 && (uint64_t)rows * per_row + 96 > 48 * 1024) rows /= 2;
            sp.rows_per_tile = rows;
            sp.lds_bytes = (uint32_t)((uint64_t)rows * per_row + 96);
          }
          if (slots) {
            sp.lds_agg_slots = slots;
            sp.lds_agg_off = (sp.lds_bytes + 15u) & ~15u;
            sp.lds_bytes = sp.lds_agg_off +
                           slots * (8 + (uint32_t)sp.n_aggs * (uint32_t)sizeof(SimpleAggAcc));
          }
          int le = dev_scan_launch(sp, regions[rg]->dev, nullptr, &ht, nullptr, eng->stream);
          if (le) { free_ht(); return SET_ERR(COPR_ERR_INTERNAL, "scan launch failed"); }
        }
        hipEventRecord(ev_b, eng->stream);
        timed = true;
        unsigned int h_err[2] = {0, 0};
        unsigned long long h_rsvd_seen[2];
        hipError_t ce = hipMemcpyAsync(h_err, ht.error, 8, hipMemcpyDeviceToHost, eng->stream);
        if (ce == hipSuccess)
          ce = hipMemcpyAsync(h_rsvd_seen, ht.rsvd_seen, 16, hipMemcpyDeviceToHost, eng->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(eng->stream);
        if (ce != hipSuccess) { free_ht(); return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(ce)); }
        if (h_err[0]) {  /* table full: grow and retry */
          free_ht();
          if (tsize >= (1u << 27)) return SET_ERR(COPR_ERR_OOM, "too many groups");
          tsize <<= 4;
          continue;
        }
        if (h_err[1]) { free_ht(); return SET_ERR(COPR_ERR_STORAGE, "row parse error on device"); }
        /* device-side compaction, then copy back only occupied slots */
        std::vector<long long> h_keys;
        std::vector<SimpleAggAcc> h_accs;
        std::vector<SimpleAggAcc> h_rsvd(2 * pl.sp.n_aggs);
        std::vector<unsigned long long> h_ext;
        std::vector<unsigned long long> h_rsvd_ext(2 * pl.sp.n_aggs * 2, 0);
        int ng = dev_ht_compact(ht, tsize, pl.sp.n_aggs, eng->stream,
                                &h_keys, &h_accs,
                                any_dec ? &h_ext : nullptr);
        ce = hipMemcpy(h_rsvd.data(), ht.reserved,
                       2 * pl.sp.n_aggs * sizeof(SimpleAggAcc),
                       hipMemcpyDeviceToHost);
        if (ce == hipSuccess && ht.rsvd_ext)
          ce = hipMemcpy(h_rsvd_ext.data(), ht.rsvd_ext,
                         2 * pl.sp.n_aggs * 16, hipMemcpyDeviceToHost);
        /* buffers stay cached on the engine for the next request */
        if (ng == -2) return SET_ERR(COPR_ERR_OOM, "table compact alloc");
        if (ng < 0 || ce != hipSuccess)
          return SET_ERR(COPR_ERR_INTERNAL, "table compact failed");
        if (pl.group_multi) {
          /* a group id is never INT64_MIN or NULL: reserved[] stays empty */
          copr_status est =
              emit_multi(h_keys.data(), h_keys.size(), h_accs.data(),
                         any_dec ? h_ext.data() : nullptr);
          if (est != COPR_OK) return est;
          break;
        }
        /* encode rows: occupied slots + reserved groups */
        size_t n_out_cols = pl.out_schema.size();
        bool enc_err = false;
        auto emit_group = [&](const SimpleAggAcc *accs, bool gnull,
                              int64_t gkey, const unsigned long long *gext) {
          std::vector<std::vector<uint8_t>> cols(n_out_cols);
          encode_agg_row(pl, accs, true, gnull, gkey, &cols, gext, &enc_err);
          for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
            uint32_t off = req->output_offsets[oo];
            if (off < n_out_cols)
              resp.insert(resp.end(), cols[off].begin(), cols[off].end());
          }
          n_rows_out++;
        };
        for (size_t s = 0; s < h_keys.size(); s++)
          emit_group(&h_accs[s * pl.sp.n_aggs], false, h_keys[s],
                     any_dec ? &h_ext[s * pl.sp.n_aggs * 2] : nullptr);
        if (h_rsvd_seen[0])
          emit_group(&h_rsvd[0], false, INT64_MIN,
                     any_dec ? &h_rsvd_ext[0] : nullptr);
        if (h_rsvd_seen[1])
          emit_group(&h_rsvd[pl.sp.n_aggs], true, 0,
                     any_dec ? &h_rsvd_ext[pl.sp.n_aggs * 2] : nullptr);
        if (enc_err)
          return SET_ERR(COPR_ERR_STORAGE,
                         "decimal sum overflow (Res::Overflow)");
        break;
      }
    }
  } else {
    /* ---- project mode ---- */
    for (uint32_t rg = 0; rg < n_regions && n_rows_out < pl.limit; rg++) {
      copr_region *r = regions[rg];
      uint64_t n = r->dev.n_kv;
      ProjectOut po{};
      hipError_t e = hipSuccess;
      size_t cells_b = (size_t)n * pl.sp.n_out * 8;
      if (e == hipSuccess) e = hipMalloc((void **)&po.cells, cells_b ? cells_b : 8);
      if (e == hipSuccess) e = hipMalloc((void **)&po.handles, n * 8);
      if (e == hipSuccess) e = hipMalloc((void **)&po.keep, n + 8);
      if (e == hipSuccess) e = hipMalloc((void **)&po.error, 8);
      if (e == hipSuccess && pl.sp.has_filter) {
        e = hipMalloc((void **)&po.filt_vals, n * 8 + 8);
        if (e == hipSuccess) e = hipMalloc((void **)&po.filt_state, n + 8);
      }
      if (e == hipSuccess && pl.sp.dec2_col_id) {
        e = hipMalloc((void **)&po.dec2_vals, n * 8 + 8);
        if (e == hipSuccess) e = hipMalloc((void **)&po.dec2_state, n + 8);
      }
      auto free_po = [&]() {
        hipFree(po.cells); hipFree(po.handles); hipFree(po.keep); hipFree(po.error);
        hipFree(po.filt_vals); hipFree(po.filt_state);
        hipFree(po.dec2_vals); hipFree(po.dec2_state);
      };
      if (e != hipSuccess) { free_po(); return SET_ERR(COPR_ERR_OOM, "project alloc"); }
      hipMemsetAsync(po.keep, 0, n + 8, eng->stream);
      hipMemsetAsync(po.error, 0, 8, eng->stream);
      ScanPlan sp = pl.sp;
      pick_tiling(r->dev, &sp);
      int le = dev_scan_launch(sp, r->dev, nullptr, nullptr, &po, eng->stream);
      if (le) { free_po(); return SET_ERR(COPR_ERR_INTERNAL, "scan launch failed"); }

      /* ---- device TypeChunk fast path (kernels.hip dev_chunk_encode):
         single region, table or index project, every output column
         chunk-encodes as an 8-byte fixed value. Skips the span-stream +
         cell-directory D2H and the serial host datum->chunk re-encode.
         Any row the device cannot encode falls back to the host path
         below (bit-identical either way — tests compare both). */
      if (req->encode_type == 1 && n_regions == 1) {
        const char *dc_env = getenv("COPR_DEV_CHUNK");
        bool dc_on = !(dc_env && dc_env[0] == '0');
        std::vector<copr::ChunkColSpec> specs(req->n_output_offsets);
        bool eligible = dc_on && req->n_output_offsets > 0;
        for (uint32_t oo = 0; eligible && oo < req->n_output_offsets; oo++) {
          uint32_t off = req->output_offsets[oo];
          if (off >= (uint32_t)pl.sp.n_out || off >= pl.out_schema.size() ||
              off >= pl.cols.size()) { eligible = false; break; }
          copr::ChunkColSpec &cs = specs[oo];
          memset(&cs, 0, sizeof(cs));
          switch (pl.out_schema[off].tp) {
            case COPR_TP_TINY: case COPR_TP_SHORT: case COPR_TP_INT24:
            case COPR_TP_LONG: case COPR_TP_LONGLONG: case COPR_TP_YEAR:
              cs.is_real = 0; break;
            case COPR_TP_DOUBLE: cs.is_real = 1; break;
            case COPR_TP_DURATION: cs.is_real = 2; break;
            default: eligible = false;
          }
          if (!eligible) break;
          if (pl.sp.out_is_handle[off]) {
            cs.kind = 1;
          } else if ((int)off == pl.dec2_col_offset && pl.sp.dec2_col_id) {
            cs.kind = 3;
            cs.missing_null = pl.sp.dec2_missing_null;
            cs.missing_val = pl.sp.dec2_missing_val;
          } else if ((int)off == pl.filter_col_offset && pl.sp.has_filter) {
            cs.kind = 2;
            cs.missing_null = pl.sp.filter_missing_null;
            cs.missing_val = pl.sp.filter_missing_val;
          } else {
            cs.kind = 0;
            cs.j = (int32_t)off;
            const CoprColumnInfo &ci = pl.cols[off];
            cs.uns = (ci.ft.flag & COPR_FLAG_UNSIGNED) ? 1 : 0;
            if (ci.default_val && ci.default_val_len) {
              int64_t dv;
              int dr = host_decode_int_datum(ci.default_val,
                                             ci.default_val_len, &dv);
              if (dr < 0) { eligible = false; break; }
              cs.missing_null = dr == 1 ? 1 : 0;
              cs.missing_val = dv;
            } else if (!(ci.ft.flag & COPR_FLAG_NOT_NULL)) {
              cs.missing_null = 1;
            } else {
              /* NOT NULL without default: a missing cell must raise the
                 reference's error -> host path */
              eligible = false;
            }
          }
        }
        if (eligible) {
          std::vector<uint8_t> dk(n);
          unsigned int derr[2] = {0, 0};
          hipError_t de = hipMemcpyAsync(dk.data(), po.keep, n,
                                         hipMemcpyDeviceToHost, eng->stream);
          if (de == hipSuccess)
            de = hipMemcpyAsync(derr, po.error, 8, hipMemcpyDeviceToHost,
                                eng->stream);
          if (de == hipSuccess) de = hipStreamSynchronize(eng->stream);
          if (de != hipSuccess) {
            free_po();
            return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(de));
          }
          if (derr[1]) {
            free_po();
            return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");
          }
          /* paging + chunk ladder over the keep flags (same walk as the
             host path below; runner.rs:917-943) */
          uint64_t scan_end_l = n, resume_l = UINT64_MAX;
          if (req->paging_size) {
            uint64_t bs = 32, pos = 0, outcnt = 0;
            while (pos < n) {
              uint64_t e2 = std::min(n, pos + bs);
              for (uint64_t i = pos; i < e2; i++) outcnt += dk[i] ? 1 : 0;
              pos = e2;
              if (outcnt >= req->paging_size) break;
              if (bs < 1024) bs *= 2;
            }
            if (pos < n) { scan_end_l = pos; resume_l = pos; }
          }
          std::vector<uint64_t> cr_l;
          {
            uint64_t bs = 32, pos2 = 0, limit_left =
                pl.limit == UINT64_MAX ? UINT64_MAX : pl.limit - n_rows_out;
            while (pos2 < scan_end_l && limit_left) {
              uint64_t e2 = std::min(scan_end_l, pos2 + bs);
              uint64_t cnt2 = 0;
              for (uint64_t i = pos2; i < e2 && cnt2 < limit_left; i++)
                cnt2 += dk[i] ? 1 : 0;
              if (cnt2) cr_l.push_back(cnt2);
              if (limit_left != UINT64_MAX) limit_left -= cnt2;
              pos2 = e2;
              if (bs < 1024) bs *= 2;
            }
          }
          std::vector<uint8_t> chunk_bytes;
          int rc = copr::dev_chunk_encode(po, r->dev,
                                          pl.sp.index_mode != 0, scan_end_l,
                                          specs.data(),
                                          (int)req->n_output_offsets,
                                          pl.sp.n_out, cr_l, eng->stream,
                                          &chunk_bytes);
          if (rc == 0) {
            free_po();
            resp.insert(resp.end(), chunk_bytes.begin(), chunk_bytes.end());
            for (uint64_t cn : cr_l) n_rows_out += cn;
            out->resume_row = resume_l;
            dev_chunked = true;
            continue;
          }
          /* -3 (a row needs host decode) or alloc/hip trouble: fall
             through to the host path, which recomputes everything */
        }
      }
      std::vector<uint8_t> h_keep(n);
      std::vector<unsigned long long> h_cells((size_t)n * pl.sp.n_out);
      std::vector<long long> h_handles;
      unsigned int h_err[2] = {0, 0};
      hipError_t ce = hipMemcpyAsync(h_keep.data(), po.keep, n, hipMemcpyDeviceToHost, eng->stream);
      if (ce == hipSuccess && pl.sp.n_out)
        ce = hipMemcpyAsync(h_cells.data(), po.cells, cells_b, hipMemcpyDeviceToHost, eng->stream);
      bool any_handle = false;
      for (int j = 0; j < pl.sp.n_out; j++) any_handle |= pl.sp.out_is_handle[j] != 0;
      if (ce == hipSuccess && any_handle) {
        h_handles.resize(n);
        ce = hipMemcpyAsync(h_handles.data(), po.handles, n * 8, hipMemcpyDeviceToHost, eng->stream);
      }
      std::vector<long long> h_fvals;
      std::vector<uint8_t> h_fstate;
      if (ce == hipSuccess && pl.sp.has_filter) {
        h_fvals.resize(n);
        h_fstate.resize(n);
        ce = hipMemcpyAsync(h_fvals.data(), po.filt_vals, n * 8, hipMemcpyDeviceToHost, eng->stream);
        if (ce == hipSuccess)
          ce = hipMemcpyAsync(h_fstate.data(), po.filt_state, n, hipMemcpyDeviceToHost, eng->stream);
      }
      std::vector<long long> h_d2vals;
      std::vector<uint8_t> h_d2state;
      if (ce == hipSuccess && pl.sp.dec2_col_id) {
        h_d2vals.resize(n);
        h_d2state.resize(n);
        ce = hipMemcpyAsync(h_d2vals.data(), po.dec2_vals, n * 8, hipMemcpyDeviceToHost, eng->stream);
        if (ce == hipSuccess)
          ce = hipMemcpyAsync(h_d2state.data(), po.dec2_state, n, hipMemcpyDeviceToHost, eng->stream);
      }
      if (ce == hipSuccess)
        ce = hipMemcpyAsync(h_err, po.error, 8, hipMemcpyDeviceToHost, eng->stream);
      if (ce == hipSuccess) ce = hipStreamSynchronize(eng->stream);
      free_po();
      if (ce != hipSuccess) return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(ce));
      if (h_err[1]) return SET_ERR(COPR_ERR_STORAGE, "row parse error on device");

      /* pull the SPAN-SOURCE bytes for kept rows (whole buffer if small):
         index project spans reference the KEY stream */
      const bool idxp = pl.sp.index_mode != 0;
      const uint8_t *d_span_src = idxp ? r->dev.d_keys : r->dev.d_vals;
      const uint64_t span_bytes = idxp ? r->dev.key_bytes : r->dev.val_bytes;
      const std::vector<uint64_t> &span_offs =
          idxp ? r->h_key_offs : r->h_val_offs;
      std::vector<uint8_t> h_vals;
      bool whole = span_bytes <= (256u << 20);
      if (whole) {
        h_vals.resize(span_bytes);
        HIP_TRY(hipMemcpy(h_vals.data(), d_span_src, span_bytes,
                          hipMemcpyDeviceToHost), "vals D2H");
      }
      /* paging (runner.rs:917-943): walk the reference's batch ladder
         (32 -> x2 -> 1024) over the keep flags and stop at the first batch
         boundary where accumulated OUTPUT rows reach paging_size */
      uint64_t scan_end = n;
      if (req->paging_size && n_regions == 1) {
        uint64_t bs = 32, pos = 0, outcnt = 0;
        while (pos < n) {
          uint64_t e2 = std::min(n, pos + bs);
          for (uint64_t i = pos; i < e2; i++) outcnt += h_keep[i] ? 1 : 0;
          pos = e2;
          if (outcnt >= req->paging_size) break;
          if (bs < 1024) bs *= 2;
        }
        if (pos < n) {
          scan_end = pos;
          out->resume_row = pos;
        }
      }
      if (req->encode_type == 1) {
        /* chunk segmentation mirrors the batch ladder over this region's
           keep flags, capped by the remaining LIMIT */
        uint64_t bs = 32, pos2 = 0, limit_left =
            pl.limit == UINT64_MAX ? UINT64_MAX : pl.limit - n_rows_out;
        while (pos2 < scan_end && limit_left) {
          uint64_t e2 = std::min(scan_end, pos2 + bs);
          uint64_t cnt2 = 0;
          for (uint64_t i = pos2; i < e2 && cnt2 < limit_left; i++)
            cnt2 += h_keep[i] ? 1 : 0;
          if (cnt2 > limit_left) cnt2 = limit_left;
          if (cnt2) chunk_rows.push_back(cnt2);
          if (limit_left != UINT64_MAX) limit_left -= cnt2;
          pos2 = e2;
          if (bs < 1024) bs *= 2;
        }
      }
      std::vector<uint8_t> rowbuf;
      auto dec_override = [&](int off) -> const copr_engine::DecOverride * {
        for (const copr_engine::DecOverride &ov : eng->topn_dec)
          if (ov.col_off == off) return &ov;
        return nullptr;
      };
      for (uint64_t i = 0; i < scan_end && n_rows_out < pl.limit; i++) {
        if (!h_keep[i]) continue;
        const uint8_t *vbase = nullptr;
        if (whole) vbase = h_vals.data();
        else {
          uint64_t vo = span_offs[i], vl = span_offs[i + 1] - vo;
          rowbuf.resize(vl);
          hipMemcpy(rowbuf.data(), d_span_src + vo, vl, hipMemcpyDeviceToHost);
          vbase = rowbuf.data() - vo;
        }
        for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
          uint32_t off = req->output_offsets[oo];
          if (off >= (uint32_t)pl.sp.n_out)
            return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad output offset");
          if (pl.sp.out_is_handle[off]) {
            enc_datum_int(&resp, h_handles[i],
                          (pl.cols[off].ft.flag & COPR_FLAG_UNSIGNED) != 0);
            continue;
          }
          if (const copr_engine::DecOverride *ov = dec_override((int)off)) {
            /* multi-key TopN order column: decoded by the order expression */
            if (i >= ov->vals.size())
              return SET_ERR(COPR_ERR_INTERNAL, "TopN key override short");
            if (ov->nulls[i]) resp.push_back(0);
            else enc_datum_int(&resp, ov->vals[i], ov->uns);
            continue;
          }
          if ((int)off == pl.dec2_col_offset && pl.sp.dec2_col_id) {
            uint8_t st8 = h_d2state[i];
            bool uns = (pl.cols[off].ft.flag & COPR_FLAG_UNSIGNED) != 0;
            bool fr = pl.sp.filter2_is_real != 0;
            if (st8 == 0) {
              if (fr) enc_datum_real(&resp, (uint64_t)h_d2vals[i]);
              else enc_datum_int(&resp, h_d2vals[i], uns);
            } else if (st8 == 1) resp.push_back(0);
            else if (pl.sp.dec2_missing_null) resp.push_back(0);
            else if (fr) enc_datum_real(&resp, (uint64_t)pl.sp.dec2_missing_val);
            else enc_datum_int(&resp, pl.sp.dec2_missing_val, uns);
            continue;
          }
          if ((int)off == pl.filter_col_offset && pl.sp.has_filter) {
            /* the predicate decoded this column in place, so its output is
               the DECODED datum (ensure_columns_decoded -> lazy_column
               Decoded encode, lazy_column.rs:165,242; vector.rs:372-383) */
            uint8_t st8 = h_fstate[i];
            bool uns = (pl.cols[off].ft.flag & COPR_FLAG_UNSIGNED) != 0;
            bool fr = pl.sp.filter_is_real != 0;
            if (st8 == 0) {
              if (fr) enc_datum_real(&resp, (uint64_t)h_fvals[i]);
              else enc_datum_int(&resp, h_fvals[i], uns);
            } else if (st8 == 1) resp.push_back(0);
            else if (pl.sp.filter_missing_null) resp.push_back(0);
            else if (fr) enc_datum_real(&resp, (uint64_t)pl.sp.filter_missing_val);
            else enc_datum_int(&resp, pl.sp.filter_missing_val, uns);
            continue;
          }
          unsigned long long cp = h_cells[i * pl.sp.n_out + off];
          uint32_t clen = (uint32_t)(cp & 0xFFFFFu);
          const bool host_dec =
              std::find(eng->host_dec_offs.begin(), eng->host_dec_offs.end(),
                        (int)off) != eng->host_dec_offs.end();
          if (host_dec && clen != 0xFFFFEu) {
            /* an int column the original request's selection decoded: the
               cell, or the default of an absent one, as a decoded datum. A v2
               cell's re-encode below is that form already. */
            const CoprColumnInfo &ci = pl.cols[off];
            const uint8_t *dp = nullptr;
            size_t dl = 0;
            if (clen == 0xFFFFFu) {
              dp = ci.default_val;
              dl = dp ? ci.default_val_len : 0;
            } else {
              uint64_t rs = span_offs[i];
              if (!(!idxp && span_offs[i + 1] - rs > 1 && vbase[rs] == 128)) {
                dp = vbase + (cp >> 20);
                dl = clen;
              }
            }
            if (dp && dl) {
              int64_t dv;
              int dr = host_decode_int_datum(dp, dl, &dv);
              if (dr < 0) return SET_ERR(COPR_ERR_STORAGE, "bad int cell");
              if (dr == 1) resp.push_back(0);
              else enc_datum_int(&resp, dv, (ci.ft.flag & COPR_FLAG_UNSIGNED) != 0);
              continue;
            }
          }
          if (clen == 0xFFFFFu) {
            /* missing column: default value or NULL
               (table_scan_executor.rs:456-483) */
            const CoprColumnInfo &ci = pl.cols[off];
            if (ci.default_val && ci.default_val_len)
              resp.insert(resp.end(), ci.default_val, ci.default_val + ci.default_val_len);
            else if (!(ci.ft.flag & COPR_FLAG_NOT_NULL))
              resp.push_back(0);
            else
              return SET_ERR(COPR_ERR_STORAGE, "missing NOT NULL column");
          } else if (clen == 0xFFFFEu) {
            resp.push_back(0);                 /* explicit v2 NULL cell */
          } else {
            uint64_t goff = cp >> 20;
            uint64_t rs = span_offs[i];
            uint64_t rl = span_offs[i + 1] - rs;
            if (!idxp && rl > 1 && vbase[rs] == 128) {
              /* v2 row: raw payload -> datum re-encode */
              const CoprColumnInfo &ci = pl.cols[off];
              if (!e_v2_cell_to_datum(ci.ft.tp, ci.ft.flag, vbase + goff,
                                      clen, &resp))
                return SET_ERR(COPR_ERR_UNSUPPORTED, "v2 cell re-encode");
            } else {
              resp.insert(resp.end(), vbase + goff, vbase + goff + clen);
            }
          }
        }
        n_rows_out++;
      }
    }
  }

  if (timed) {
    hipEventSynchronize(ev_b);
    hipEventElapsedTime(&kernel_ms, ev_a, ev_b);
  }
  if (req->encode_type == 1 && !dev_chunked) {
    if (chunk_rows.empty() && n_rows_out) {
      for (uint64_t left = n_rows_out; left;) {      /* drain: 1024/chunk */
        uint64_t b = left < 1024 ? left : 1024;
        chunk_rows.push_back(b);
        left -= b;
      }
    }
    std::vector<CoprFieldType> fts;
    for (uint32_t oo = 0; oo < req->n_output_offsets; oo++) {
      uint32_t off = req->output_offsets[oo];
      if (off >= pl.out_schema.size())
        return SET_ERR(COPR_ERR_INVALID_REQUEST, "bad output offset");
      fts.push_back(pl.out_schema[off]);
    }
    std::vector<uint8_t> chunked;
    if (!e_chunk_encode_post(resp, chunk_rows, fts, &chunked))
      return SET_ERR(COPR_ERR_UNSUPPORTED, "TypeChunk encode failed");
    resp.swap(chunked);
  }
  out->data = (uint8_t *)malloc(resp.size() ? resp.size() : 1);
  memcpy(out->data, resp.data(), resp.size());
  out->data_len = resp.size();
  out->n_rows = n_rows_out;
  out->summaries = (CoprExecSummary *)calloc(req->n_executors, sizeof(CoprExecSummary));
  out->n_summaries = req->n_executors;
  if (out->n_summaries) {
    out->summaries[out->n_summaries - 1].num_produced_rows = n_rows_out;
    out->summaries[0].time_processed_ns = (uint64_t)(kernel_ms * 1e6);
    out->summaries[0].num_iterations = 1;
  }
  return COPR_OK;
}

extern "C" void copr_result_free(CoprSelectResult *r) {
  if (!r) return;
  free(r->data); free(r->summaries);
  r->data = nullptr; r->summaries = nullptr;
}

/* ---------------- checksum ---------------- */
static void build_crc_tables(uint64_t tab[8 * 256]) {
  const uint64_t POLY = 0x42F0E1EBA9EA3693ull;
  uint64_t rpoly = 0;
  for (int i = 0; i < 64; i++)
    if (POLY & (1ull << i)) rpoly |= 1ull << (63 - i);
  for (int i = 0; i < 256; i++) {
    uint64_t crc = (uint64_t)i;
    for (int j = 0; j < 8; j++) crc = (crc >> 1) ^ ((crc & 1) ? rpoly : 0);
    tab[i] = crc;
  }
  /* tables 0..7: slice-by-8, all that k_crc64_reg reads */
  for (int t = 1; t < 8; t++)
    for (int i = 0; i < 256; i++) {
      uint64_t prev = tab[(t - 1) * 256 + i];
      tab[t * 256 + i] = tab[prev & 0xFF] ^ (prev >> 8);
    }
}

extern "C" copr_status copr_checksum(copr_engine *eng, copr_region *const *regions,
                                     uint32_t n_regions, uint64_t *checksum,
                                     uint64_t *total_kvs, uint64_t *total_bytes) {
  if (!eng) return SET_ERR(COPR_ERR_INVALID_REQUEST, "null engine");
  HIP_TRY(hipSetDevice(eng->device), "hipSetDevice");
  if (!eng->d_crc_tables) {
    uint64_t tab[8 * 256];
    build_crc_tables(tab);
    HIP_TRY(hipMalloc(&eng->d_crc_tables, sizeof(tab)), "crc tab alloc");
    HIP_TRY(hipMemcpy(eng->d_crc_tables, tab, sizeof(tab), hipMemcpyHostToDevice),
            "crc tab upload");
  }
  unsigned long long *d_xor = nullptr;
  HIP_TRY(hipMalloc(&d_xor, 8), "xor alloc");
  HIP_TRY(hipMemsetAsync(d_xor, 0, 8, eng->stream), "xor memset");
  uint64_t kvs = 0, bytes = 0;
  for (uint32_t rg = 0; rg < n_regions; rg++) {
    const DevRegion &rv = regions[rg]->dev;
    int e = dev_crc64_launch(rv, eng->d_crc_tables, d_xor, eng->stream);
    if (e) { hipFree(d_xor); return SET_ERR(COPR_ERR_INTERNAL, "crc launch failed"); }
    kvs += rv.n_kv;
    bytes += rv.key_bytes + rv.val_bytes;
  }
  unsigned long long h_xor = 0;
  hipError_t ce = hipMemcpyAsync(&h_xor, d_xor, 8, hipMemcpyDeviceToHost, eng->stream);
  if (ce == hipSuccess) ce = hipStreamSynchronize(eng->stream);
  hipFree(d_xor);
  if (ce != hipSuccess) return SET_ERR(COPR_ERR_INTERNAL, hipGetErrorString(ce));
  *checksum = h_xor;
  *total_kvs = kvs;
  *total_bytes = bytes;
  return COPR_OK;
}
