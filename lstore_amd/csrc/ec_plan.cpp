// ec_plan.cpp -- the plan service of liblstore_ec.so: et_new_plan / et_generate_plan /
// et_destroy_plan and the plan's fn-pointers (form_*), with the same arguments, return codes and
// struct contents as src/lio/erasure_tools.c; the coding matrices and their per-device images
// (encode image per plan, decode image per erasure pattern, built once and cached); and the
// device-resident core (enqueue_apply: every coding launch, for every route).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <strings.h>

#include <array>
#include <cstdio>

#include "ec_jit.h"
#include "ec_engine.h"
#include "ec_vote.h"

#include <unistd.h>

extern "C" const char *JE_method[N_JE_METHODS] = {"reed_sol_van", "reed_sol_r6_op", "cauchy_orig", "cauchy_good",
                                                  "blaum_roth",   "liberation",     "liber8tion",  "raid4"};

namespace lsec {
namespace eng {

thread_local std::string tl_err;

int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  tl_err = buf;
  return -1;
}

// Ends the process with a reason that survives it: written to fd 2 with write(2) (no stdio
// buffer to lose) and appended to the file LSEC_FATAL_LOG names, if set -- a test runner that
// captures fd 2 into a temporary file loses that file when the process aborts (VERDICT r03:
// an abort in a GPU suite run whose reason never reached the log).
[[noreturn]] void fatal(const char *fmt, ...) {
  char buf[1024];
  int n = snprintf(buf, sizeof(buf), "liblstore_ec: fatal: ");
  va_list ap;
  va_start(ap, fmt);
  n += vsnprintf(buf + n, sizeof(buf) - n - 2, fmt, ap);
  va_end(ap);
  n = std::min<int>(n, sizeof(buf) - 2);
  buf[n++] = '\n';
  if (write(2, buf, n) < 0) {
  }
  if (const char *path = getenv("LSEC_FATAL_LOG"))
    if (FILE *f = fopen(path, "a")) {
      fwrite(buf, 1, n, f);
      fclose(f);
    }
  abort();
}

int max_devs(int method, int w) {
  const bool matrix = method == REED_SOL_VAN || method == REED_SOL_R6_OP || method == CAUCHY_ORIG || method == CAUCHY_GOOD;
  return matrix && (w == 16 || w == 32) ? kMaxDevs : LSEC_MAX_DEVS;
}

PlanExt *ext_of(lio_erasure_plan_t *p) {
  if (!p) return nullptr;
  PlanExt *e = reinterpret_cast<PlanExt *>(p);
  return e->magic == kPlanMagic ? e : nullptr;
}

bool liberation_family(int method) { return method == BLAUM_ROTH || method == LIBERATION || method == LIBER8TION; }

// Which kernel applies a plan:
//   RS / r6 at w = 8 -> bytewise GF(2^8); at w = 16 / 32 -> wordwise GF(2^w)
//   Cauchy at w = 8 -> bit-sliced GF(2^8); at w = 16 / 32 -> bit-sliced GF(2^w)
//   liberation family -> generic GF(2) bitmatrix; raid4 -> bytewise XOR (w unused, raid4.c)
int kernel_kind(int method, int w) {
  if (liberation_family(method)) return w >= 2 && w <= lsec::kMaxW ? KBITMATRIX : KNONE;
  if (method == RAID4) return KBYTEWISE;
  const bool wide = (w == 16 || w == 32);
  if (w != 8 && !wide) return KNONE;
  switch (method) {
    case REED_SOL_VAN:
    case REED_SOL_R6_OP:
      return wide ? KWORDWISE : KBYTEWISE;
    case CAUCHY_ORIG:
    case CAUCHY_GOOD:
      return wide ? KBITSLICEDW : KBITSLICED;
    default:
      return KNONE;
  }
}

bool uses_u32_image(int kind) { return kind == KBITMATRIX || kind == KWORDWISE || kind == KBITSLICEDW; }
bool packet_kind(int kind) { return kind == KBITSLICED || kind == KBITMATRIX || kind == KBITSLICEDW; }

// a malloc'd int copy (the public struct's matrices are the caller's to free()) of a GF(2^8) or
// GF(2^w) matrix, or of a bitmatrix
template <typename V>
int *to_int_array(const V &v) {
  int *a = static_cast<int *>(malloc(sizeof(int) * v.size()));
  for (size_t i = 0; i < v.size(); ++i) a[i] = static_cast<int>(v[i]);
  return a;
}

// word image of an R x K GF(2^w) matrix for k_gfw_wordwise: [(r*K + j)*w + b] = M[r][j] * x^b
std::vector<uint32_t> word_image(const lsec::gfw::Mat &mat, int rows, int cols, int w) {
  std::vector<uint32_t> img(static_cast<size_t>(rows) * cols * w);
  for (int i = 0; i < rows * cols; ++i) lsec::make_word_cell(mat[i], w, &img[static_cast<size_t>(i) * w]);
  return img;
}

// bitmatrix row masks for the generic bitmatrix kernels: NW = mask_words(w) words per (row, input),
// bit x of word [((r*w+l)*k + j)*NW + q] = B[r*w+l][j*w + 32q + x]
std::vector<uint32_t> bitmatrix_masks(const int *bm, int k, int m, int w) {
  const int nw = lsec::mask_words(w);
  std::vector<uint32_t> mk(static_cast<size_t>(m) * w * k * nw, 0u);
  for (int row = 0; row < m * w; ++row)
    for (int j = 0; j < k; ++j)
      for (int x = 0; x < w; ++x)
        if (bm[static_cast<size_t>(row) * k * w + j * w + x])
          mk[(static_cast<size_t>(row) * k + j) * nw + x / 32] |= 1u << (x % 32);
  return mk;
}

// Image rows per output row and elements per (row, input) of a kernel kind's image.
int image_rows_per_output(int kind, int w) { return kind == KBITMATRIX ? w : 1; }
int image_unit(int kind, int w) {
  return kind == KBITMATRIX ? lsec::mask_words(w) : (kind == KWORDWISE || kind == KBITSLICEDW) ? w : 1;
}

// The grouped layout of ec_kernels.h for images of more than lsec::kMaxK inputs: `rows` image
// rows of K inputs x `unit` elements, row-major -> groups of kMaxK inputs, each row-major.
template <typename T>
void group_image(std::vector<T> &img, int rows, int K, int unit) {
  if (K <= lsec::kMaxK) return;
  std::vector<T> out(img.size());
  size_t o = 0;
  for (int k0 = 0; k0 < K; k0 += lsec::kMaxK) {
    const int kg = std::min(lsec::kMaxK, K - k0);
    for (int r = 0; r < rows; ++r) {
      const T *src = &img[(static_cast<size_t>(r) * K + k0) * unit];
      std::copy(src, src + static_cast<size_t>(kg) * unit, &out[o]);
      o += static_cast<size_t>(kg) * unit;
    }
  }
  img.swap(out);
}

int **schedule_array(const std::vector<std::array<int, 5>> &ops) {
  int **s = static_cast<int **>(malloc(sizeof(int *) * (ops.size() + 1)));
  for (size_t i = 0; i < ops.size(); ++i) {
    s[i] = static_cast<int *>(malloc(sizeof(int) * 5));
    std::memcpy(s[i], ops[i].data(), sizeof(int) * 5);
  }
  s[ops.size()] = static_cast<int *>(malloc(sizeof(int) * 5));
  s[ops.size()][0] = -1;
  return s;
}

// Builds the plan's public matrix objects (what erasure_tools.c's form_* routines build,
// erasure_tools.c:101-292) and the kernel's GF matrix.  `with_schedule` distinguishes
// form_encoding_matrix (matrix + bitmatrix + schedule) from form_decoding_matrix.
int form_matrices(lio_erasure_plan_t *p, bool with_schedule) {
  PlanExt *e = ext_of(p);
  if (!e) return -1;
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const int k = p->data_strips, m = p->parity_strips, w = p->w;
  lsec::gf8::Mat mat;
  switch (p->method) {
    case RAID4:
      e->impl->coding.assign(k, 1);
      e->impl->coding_ready = true;
      e->impl->coding_fast.store(true, std::memory_order_release);
      return 0;
    case REED_SOL_VAN:
    case REED_SOL_R6_OP: {
      if (!p->encode_matrix) {
        const bool r6 = p->method == REED_SOL_R6_OP;
        if (w == 8) {
          if (!(r6 ? lsec::gf8::reed_sol_r6(k, mat) : lsec::gf8::reed_sol_vandermonde(k, m, mat)))
            return fail("cannot form %s matrix for k=%d m=%d w=%d", JE_method[p->method], k, m, w);
          p->encode_matrix = to_int_array(mat);
        } else {
          lsec::gfw::Mat wm;
          const bool ok = (w == 16 || w == 32) &&
                          (r6 ? lsec::gfw::reed_sol_r6(k, w, wm) : lsec::gfw::reed_sol_vandermonde(k, m, w, wm));
          if (!ok) return fail("cannot form %s matrix for k=%d m=%d w=%d", JE_method[p->method], k, m, w);
          p->encode_matrix = to_int_array(wm);
        }
      }
      break;
    }
    case CAUCHY_ORIG:
    case CAUCHY_GOOD: {
      if (!p->encode_matrix) {
        const bool orig = p->method == CAUCHY_ORIG;
        if (w == 8) {
          if (!(orig ? lsec::gf8::cauchy_original(k, m, mat) : lsec::gf8::cauchy_good(k, m, mat)))
            return fail("cannot form %s matrix for k=%d m=%d w=%d", JE_method[p->method], k, m, w);
          p->encode_matrix = to_int_array(mat);
          p->encode_bitmatrix = to_int_array(lsec::gf8::to_bitmatrix(k, m, mat));
        } else {
          lsec::gfw::Mat wm;
          const bool ok = (w == 16 || w == 32) &&
                          (orig ? lsec::gfw::cauchy_original(k, m, w, wm) : lsec::gfw::cauchy_good(k, m, w, wm));
          if (!ok) return fail("cannot form %s matrix for k=%d m=%d w=%d", JE_method[p->method], k, m, w);
          p->encode_matrix = to_int_array(wm);
          p->encode_bitmatrix = to_int_array(lsec::gfw::to_bitmatrix(k, m, w, wm));
        }
      }
      break;
    }
    case BLAUM_ROTH:
    case LIBERATION:
    case LIBER8TION: {
      if (!p->encode_bitmatrix) {
        std::vector<int> bm = p->method == LIBERATION   ? lsec::gf8::liberation_bitmatrix(k, w)
                              : p->method == BLAUM_ROTH ? lsec::gf8::blaum_roth_bitmatrix(k, w)
                                                        : lsec::gf8::liber8tion_bitmatrix(k);
        if (bm.empty()) return fail("cannot form %s bitmatrix for k=%d w=%d", JE_method[p->method], k, w);
        p->encode_bitmatrix = to_int_array(bm);
      }
      break;
    }
    default:
      return fail("invalid method %d", p->method);
  }
  const bool bitmatrix_code = p->method == CAUCHY_ORIG || p->method == CAUCHY_GOOD || liberation_family(p->method);
  if (bitmatrix_code && with_schedule && !p->encode_schedule) {
    std::vector<int> bm(p->encode_bitmatrix, p->encode_bitmatrix + static_cast<size_t>(k) * m * w * w);
    p->encode_schedule = schedule_array(lsec::gf8::smart_schedule(k, m, w, bm));
  }
  if (e->impl->coding_ready) return 0;
  const int kind = kernel_kind(p->method, w);
  if (kind == KBITMATRIX) {
    if (!p->encode_bitmatrix) return 0;
    e->impl->enc_masks = bitmatrix_masks(p->encode_bitmatrix, k, m, w);
    group_image(e->impl->enc_masks, m * w, k, lsec::mask_words(w));
    e->impl->coding_ready = true;
    e->impl->coding_fast.store(true, std::memory_order_release);
  } else if (p->encode_matrix) {
    const int rows = (p->method == REED_SOL_R6_OP) ? 2 : m;
    if (kind == KWORDWISE || kind == KBITSLICEDW) {
      e->impl->coding_w.resize(static_cast<size_t>(rows) * k);
      for (size_t i = 0; i < e->impl->coding_w.size(); ++i) e->impl->coding_w[i] = static_cast<uint32_t>(p->encode_matrix[i]);
      e->impl->enc_masks = word_image(e->impl->coding_w, rows, k, w);
      group_image(e->impl->enc_masks, rows, k, w);
    } else {
      e->impl->coding.resize(static_cast<size_t>(rows) * k);
      for (size_t i = 0; i < e->impl->coding.size(); ++i) e->impl->coding[i] = static_cast<uint8_t>(p->encode_matrix[i]);
    }
    e->impl->coding_ready = true;
    e->impl->coding_fast.store(true, std::memory_order_release);
  }
  return 0;
}

// fn-pointer versions, with the reference's return-code behaviour
int fp_form_encoding(lio_erasure_plan_t *p) {
  if (!p) return -1;
  return form_matrices(p, true);
}

int fp_form_decoding(lio_erasure_plan_t *p) {
  if (!p) return -1;
  // "Already formed so skip step": every *_form_coding_matrix returns 0 at once when its
  // matrix (Cauchy) or bitmatrix (liberation family) exists (erasure_tools.c:137, :152, :169,
  // :184, :198), whatever the schedule
  const bool cauchy = p->method == CAUCHY_ORIG || p->method == CAUCHY_GOOD;
  const bool formed = cauchy ? p->encode_matrix != nullptr : liberation_family(p->method) && p->encode_bitmatrix != nullptr;
  const int rc = form_matrices(p, false);
  if (rc || formed) return rc;
  // ... and -1 when it has just formed it while the schedule is still unset (:142, :159,
  // :176, :190, :204)
  if ((cauchy || liberation_family(p->method)) && !p->encode_schedule) return -1;
  return 0;
}

int ensure_coding(PlanExt *e) {
  if (e->impl->coding_fast.load(std::memory_order_acquire)) return 0;
  {
    std::lock_guard<std::mutex> lk(e->impl->mu);
    if (e->impl->coding_ready) return 0;
  }
  return form_matrices(&e->pub, true);
}

void host_cells(const lsec::gf8::Mat &mat, int rows, int cols, std::vector<CoefCell> &cells) {
  cells.resize(static_cast<size_t>(rows) * cols);
  for (int i = 0; i < rows * cols; ++i) lsec::make_cell(mat[i], cells[i]);
  // flag plain-XOR rows (any launch whose first row is one takes the XOR-row kernel path)
  for (int r = 0; r < rows; ++r)
    if (row_all_ones(mat.data() + static_cast<size_t>(r) * cols, cols)) cells[static_cast<size_t>(r) * cols].pad |= lsec::kCellXorRow;
}

int upload(const void *host, size_t nbytes, const char *what, void **out) {
  void *d = nullptr;
  HIP_OK(hipMalloc(&d, nbytes));
  hipError_t err = hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(d);
    return fail("%s: %s", what, hipGetErrorString(err));
  }
  *out = d;
  return 0;
}

int DevImage::get(int dev, const void *host, size_t nbytes, const char *what,
                  const std::function<void(const void *)> &on_first_upload, const void **out) {
  auto it = by_dev_.find(dev);
  if (it == by_dev_.end()) {
    void *d = nullptr;
    if (upload(host, nbytes, what, &d)) return -1;
    it = by_dev_.emplace(dev, d).first;
    if (on_first_upload) {
      bound_ = true;
      on_first_upload(d);
    }
  }
  *out = it->second;
  return 0;
}

void DevImage::drop(int dev) {
  const auto it = by_dev_.find(dev);
  if (it == by_dev_.end()) return;
  if (bound_) lsec::jit::unbind(it->second);
  (void)hipFree(it->second);
  by_dev_.erase(it);
}

void DevImage::release() {
  for (auto &kv : by_dev_) {
    if (bound_) lsec::jit::unbind(kv.second);  // before the address can be handed out again
    (void)hipSetDevice(kv.first);
    (void)hipFree(kv.second);
  }
  by_dev_.clear();
}

// The network of an R x K image just uploaded to `d`, compiled in the background from what the kind's
// generator reads: the GF(2^8) rows, the GF(2^w) rows or the row masks.
void bind_network(int kind, const void *d, const uint8_t *gf8_rows, const uint32_t *gfw_rows, const uint32_t *masks, int R, int K,
                  int w, int packet) {
  if (kind == KBYTEWISE) {  // RS / r6 at w = 8, raid4: an XOR network for the wide codes
    lsec::jit::bind(d, gf8_rows, R, K);
  } else if (kind == KBITSLICED) {  // Cauchy w = 8: a packet network (A/B knob)
    std::vector<uint32_t> c32(gf8_rows, gf8_rows + static_cast<size_t>(R) * K);
    lsec::jit::bind_pkt_field(d, c32.data(), R, K, 8, packet);
  } else if (kind == KWORDWISE) {  // RS / r6 at w = 16 / 32: a bit-sliced network
    lsec::jit::bind_w(d, gfw_rows, R, K, w);
  } else if (kind == KBITMATRIX) {  // liberation family: a packet network
    lsec::jit::bind_pkt(d, masks, R, K, w, packet);
  } else if (kind == KBITSLICEDW) {  // Cauchy at w = 16 / 32: the same
    lsec::jit::bind_pkt_field(d, gfw_rows, R, K, w, packet);
  }
}

// What an R x K image is built from.  `u32`: the host image `masks` as it is; else CoefCell[R][K] of gf8_rows.
// binds: a fresh upload gets the kind's network (bind_network).
struct CoefSource {
  int kind;
  bool u32, binds;
  const lsec::gf8::Mat &gf8_rows;
  const lsec::gfw::Mat &gfw_rows;
  const std::vector<uint32_t> &masks;
  int R, K;
};

// the image on device `dev`, the current one: built and uploaded at its first use there (the plan's mutex is held)
int coef_image(const PlanExt *e, DevImage &img, int dev, const CoefSource &c, const void **out) {
  if ((*out = img.find(dev))) return 0;
  std::vector<CoefCell> h;
  if (!c.u32) {
    host_cells(c.gf8_rows, c.R, c.K, h);
    group_image(h, c.R, c.K, 1);
  }
  std::function<void(const void *)> bind;
  if (c.binds)
    bind = [&](const void *d) {
      bind_network(c.kind, d, c.gf8_rows.data(), c.gfw_rows.data(), c.masks.data(), c.R, c.K, e->pub.w, e->pub.packet_size);
    };
  return c.u32 ? img.get(dev, c.masks.data(), sizeof(uint32_t) * c.masks.size(), "hipMemcpy(masks)", bind, out)
               : img.get(dev, h.data(), sizeof(CoefCell) * h.size(), "hipMemcpy(cells)", bind, out);
}

// output rows of the encode image (m; 2 for r6, 1 for raid4)
int encode_rows(const PlanExt *e) {
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  if (kind == KBITMATRIX) return e->pub.parity_strips;
  if (kind == KWORDWISE || kind == KBITSLICEDW) return static_cast<int>(e->impl->coding_w.size()) / e->pub.data_strips;
  return static_cast<int>(e->impl->coding.size()) / e->pub.data_strips;
}

// encode image on the current device: CoefCell[m][k] (matrix codes at w = 8, raid4), row masks
// (bitmatrix) or word products (matrix codes at w = 16 / 32)
int encode_image(PlanExt *e, const void **out) {
  if (ensure_coding(e)) return -1;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  if (dev >= 0 && dev < kFastDevs)
    if (const void *f = e->impl->enc_fast[dev].load(std::memory_order_acquire)) {
      *out = f;
      return 0;
    }
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  const CoefSource src = {kind,           uses_u32_image(kind), true, e->impl->coding, e->impl->coding_w, e->impl->enc_masks,
                          encode_rows(e), e->pub.data_strips};
  const int rc = coef_image(e, e->impl->enc_image, dev, src, out);
  if (rc == 0 && dev >= 0 && dev < kFastDevs) e->impl->enc_fast[dev].store(*out, std::memory_order_release);
  return rc;
}

int encode_job(PlanExt *e, CodingJob *job) {
  if (encode_image(e, &job->image)) return -1;
  const int k = e->pub.data_strips;
  job->kind = kernel_kind(e->pub.method, e->pub.w);
  job->R = encode_rows(e);
  job->in_ids.resize(k);
  job->out_ids.resize(job->R);
  for (int j = 0; j < k; ++j) job->in_ids[j] = j;
  for (int r = 0; r < job->R; ++r) job->out_ids[r] = k + r;
  job->gf8_rows = uses_u32_image(job->kind) ? nullptr : e->impl->coding.data();
  return 0;
}

// Parses a -1 terminated erasure list.  Returns 0 with the sorted distinct ids, 1 if the
// list is empty (nothing to do), -1 if unrecoverable / invalid.
int parse_erasures(const lio_erasure_plan_t *p, const int *erasures, std::vector<int> &ids) {
  const int k = p->data_strips, m = p->parity_strips;
  ids.clear();
  if (!erasures) return fail("erasures is NULL");
  int listed = 0;
  for (int i = 0; erasures[i] != -1; ++i) {
    const int x = erasures[i];
    if (x < 0 || x >= k + m) return fail("erasure id %d out of range 0..%d", x, k + m - 1);
    ++listed;
    if (std::find(ids.begin(), ids.end(), x) == ids.end()) ids.push_back(x);
    if (listed > 4 * (k + m)) return fail("erasure list not terminated");
  }
  std::sort(ids.begin(), ids.end());
  if (p->method == RAID4 && listed > 1) return fail("raid4 recovers one device (raid4.c:47)");
  if (static_cast<int>(ids.size()) > m) return fail("%zu erasures exceed m=%d", ids.size(), m);
  if (ids.empty()) return 1;
  return 0;
}

int decode_entry_locked(PlanExt *e, const std::vector<int> &ids, int dev, DecodeEntry **out, const void **cells);

// decode entry (host plan + device cells on the current device).  Entries are never moved or
// freed before the plan is destroyed, so each thread keeps its last lookup and repeats of it
// (a degraded read decodes the same pattern stripe after stripe) skip the plan mutex.
int decode_entry(PlanExt *e, const std::vector<int> &ids, DecodeEntry **out, const void **cells) {
  if (ensure_coding(e)) return -1;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  struct Last {
    unsigned long long serial = 0;
    int dev = -1;
    std::vector<int> ids;
    DecodeEntry *ent = nullptr;
    const void *cells = nullptr;
  };
  thread_local Last last;
  if (last.serial == e->impl->serial && last.dev == dev && last.ids == ids) {
    *out = last.ent;
    *cells = last.cells;
    return 0;
  }
  int rc;
  {
    std::lock_guard<std::mutex> lk(e->impl->mu);
    rc = decode_entry_locked(e, ids, dev, out, cells);
  }
  if (rc == 0) {
    last.serial = e->impl->serial;
    last.dev = dev;
    last.ids = ids;
    last.ent = *out;
    last.cells = *cells;
  }
  return rc;
}

// the pattern's host plan (survivors, erased ids, decode rows / masks): built once, kept in
// decode_cache; no device is touched
int decode_host_locked(PlanExt *e, const std::vector<int> &ids, DecodeEntry **out) {
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  auto it = e->impl->decode_cache.find(ids);
  if (it == e->impl->decode_cache.end()) {
    DecodeEntry ent;
    const int k = e->pub.data_strips;
    if (kind == KWORDWISE || kind == KBITSLICEDW) {
      const int w = e->pub.w;
      const int m = static_cast<int>(e->impl->coding_w.size()) / k;
      lsec::gfw::DecodePlan wp;
      if (!lsec::gfw::make_decode(k, m, w, e->impl->coding_w, ids, wp)) return fail("decoding matrix is singular");
      ent.dp.survivors = wp.survivors;
      ent.dp.erased = wp.erased;
      ent.masks = word_image(wp.rows, static_cast<int>(wp.erased.size()), k, w);
      group_image(ent.masks, static_cast<int>(wp.erased.size()), k, w);
      ent.xor_only = std::all_of(wp.rows.begin(), wp.rows.end(), [](uint32_t c) { return c <= 1u; });
      if (ent.xor_only) ent.dp.rows.assign(wp.rows.begin(), wp.rows.end());  // 0 / 1 as GF(2^8) cells
      ent.wrows.assign(wp.rows.begin(), wp.rows.end());
    } else if (kind == KBITMATRIX) {
      const lio_erasure_plan_t *p = &e->pub;
      // solves for the lost data bits only (gf8.cpp make_bit_decode): milliseconds even for the
      // widest liberation plans (k = 254, w = 257), where inverting the whole survivor bitmatrix
      // as jerasure_invert_bitmatrix does (jerasure.c:1049-1104) would take hours
      std::vector<int> bm(p->encode_bitmatrix, p->encode_bitmatrix + static_cast<size_t>(k) * p->parity_strips * p->w * p->w);
      if (!lsec::gf8::make_bit_decode(k, p->parity_strips, p->w, bm, ids, ent.dp, ent.masks))
        return fail("decoding bitmatrix is singular");
      group_image(ent.masks, static_cast<int>(ent.dp.erased.size()) * p->w, k, lsec::mask_words(p->w));
    } else {
      const int m = static_cast<int>(e->impl->coding.size()) / k;
      if (!lsec::gf8::make_decode(k, m, e->impl->coding, ids, ent.dp)) return fail("decoding matrix is singular");
      ent.xor_only = std::all_of(ent.dp.rows.begin(), ent.dp.rows.end(), [](int c) { return c == 0 || c == 1; });
    }
    it = e->impl->decode_cache.emplace(ids, std::move(ent)).first;
  }
  *out = &it->second;
  return 0;
}

int decode_entry_locked(PlanExt *e, const std::vector<int> &ids, int dev, DecodeEntry **out, const void **cells) {
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  if (decode_host_locked(e, ids, out)) return -1;
  DecodeEntry &ent = **out;
  // a u32 kind's XOR-only entry takes cells (decode_job sends it to the bytewise kernel), and no entry that only XORs binds a network
  const CoefSource src = {kind,      uses_u32_image(kind) && !ent.xor_only,      !ent.xor_only,     ent.dp.rows,
                          ent.wrows, ent.masks, static_cast<int>(ent.dp.erased.size()), e->pub.data_strips};
  return coef_image(e, ent.image, dev, src, cells);
}

// A decode that only XORs survivors (a lost data shard rebuilt from P0, whose Cauchy-good /
// RS row is all ones) is layout- and field-agnostic, so Cauchy packets and GF(2^16) / GF(2^32)
// words go through the bytewise kernel's plain-XOR path (0 / 1 cells) instead.
int decode_job(PlanExt *e, const std::vector<int> &ids, CodingJob *job) {
  DecodeEntry *ent = nullptr;
  if (decode_entry(e, ids, &ent, &job->image)) return -1;
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  const bool field = kind == KBITSLICED || kind == KWORDWISE || kind == KBITSLICEDW;
  job->kind = field && ent->xor_only ? KBYTEWISE : kind;
  job->R = static_cast<int>(ent->dp.erased.size());
  job->in_ids = ent->dp.survivors;
  job->out_ids = ent->dp.erased;
  job->gf8_rows = uses_u32_image(job->kind) ? nullptr : ent->dp.rows.data();
  return 0;
}

int check_geometry(const lio_erasure_plan_t *p, long long block_size) {
  const int k = p->data_strips, m = p->parity_strips;
  const int lim = max_devs(p->method, p->w);
  if (k < 1 || m < 1 || k + m > lim) return fail("k=%d m=%d: k+m outside 2..%d (w=%d)", k, m, lim, p->w);
  if (block_size < 0 || block_size % 8 != 0) return fail("block_size %lld is not a multiple of 8", block_size);
  const int kind = kernel_kind(p->method, p->w);
  if (kind == KNONE)
    return fail("method %s (w=%d) has no GPU kernel in this build", JE_method[p->method], p->w);
  if (packet_kind(kind)) {
    const long long sp = static_cast<long long>(p->w) * p->packet_size;
    if (p->packet_size <= 0 || p->packet_size % 4 != 0 || block_size % sp != 0)
      return fail("block_size %lld is not a multiple of w*packet_size = %lld", block_size, sp);
  }
  if (liberation_family(p->method) && m != 2) return fail("%s needs m == 2", JE_method[p->method]);
  return 0;
}

// Cauchy at w = 8 (KBITSLICED): the generic bit-sliced kernel or the compiled packet network, by
// shape.  Round 6 (profiles/r06_v13_cauchy8_kernels_ab.txt: every c5 shape at C = 1, 4, 8 MiB, one
// allocation each, interleaved): since the bit-sliced kernel took the work-sharing tail (round 5)
// and the XCD tile phase (round 6), neither of which the networks have, it beats the network on
// every shape with R <= 4 by 0.3-2.5 % -- at 4 dwords per lane from K = 16, and from K = 10 at
// chunks of 4 MiB and up; 1 dword otherwise -- while the network keeps (20+6) (R = 6; up to 3.8 %
// ahead at 4 MiB).  0: the network (where one is compiled), else the bit-sliced kernel's dwords per
// lane.  lsec_test_set_cauchy8_policy(1) gives the network every shape it has one for (tests).
std::atomic<int> g_c8_policy{0};

int cauchy8_bitsliced_dw(int K, int R, long long size) {
  if (g_c8_policy.load(std::memory_order_relaxed) == 1 || R > 4) return 0;
  if (K >= 16 || (K >= 10 && size >= (4LL << 20))) return 4;
  return 1;
}

// Stripes per launch of chunks of C bytes: batches split so that the indices of their tiles (of
// tile_bytes: 4096, or the stripe-magic calls' 8192) stay 32-bit.  With `split`,
// lsec_test_set_pattern_split can lower it: the patterned calls, the repair behind a locate, every
// launch of the rotated check and locate, the parity update and the rotated encode and update, and the
// check with the magics, rotated or not.
std::atomic<int> g_pattern_split{0};  // stripes per launch, 0 = the 32-bit tile limit only

long long launch_stripes(long long C, bool split, long long tile_bytes) {
  long long per = std::max(1LL, (1LL << 30) / std::max(1LL, C / tile_bytes + 1));
  const int hook = split ? g_pattern_split.load(std::memory_order_relaxed) : 0;
  if (hook > 0) per = std::min<long long>(per, hook);
  return per;
}

// What enqueue_apply hands launch_bitsliced as its preference: Cauchy w = 8 under the automatic policy takes the
// shape's dwords per lane (cauchy8_bitsliced_dw; 0 = the network, and one dword where none is ready)
int apply_dw_pref(int kind, int K, int R, int w, long long size, int bs_variant) {
  return kind == KBITSLICED && w == 8 && bs_variant == 0 ? cauchy8_bitsliced_dw(K, R, size) : 0;
}

// The forms one unsplit K x R call launches from the table kernels (no network ready, or none wanted), in order:
// lsec_encode_magic_dev's one fused launch where it fuses (`magic`), else enqueue_apply's launches -- for
// lsec_encode_magic_dev then followed by the magic pass, which is not of this family.  row_ones[r]: row r of the
// matrix is all ones (null: none is).  It walks for_apply_launches and asks predict_apply_launch, as the launches do.
int predict_apply(int kind, int K, int R, int w, int packet, long long size, bool magic, int bw_variant, int bs_variant,
                  const unsigned char *row_ones, std::vector<lsec::ApplyForm> &out) {
  out.clear();
  const auto one = [&](int kg, int rn, bool acc, bool mg, int dw_pref, bool ones) {
    lsec::ApplyForm f;
    if (!lsec::predict_apply_launch(kind, kg, rn, w, packet, acc, mg, dw_pref, bw_variant, bs_variant, ones, &f))
      return fail("no kernel of kind %d for K=%d R=%d w=%d packet=%d", kind, kg, rn, w, packet);
    out.push_back(f);
    return 0;
  };
  if (kind < KBYTEWISE || kind > KBITSLICEDW || K < 1 || R < 1) return fail("kind %d K=%d R=%d", kind, K, R);
  if (magic && encode_magic_fuses(kind, K, R)) return one(K, R, false, true, 0, row_ones && row_ones[0]);
  const int dw_pref = apply_dw_pref(kind, K, R, w, size, bs_variant);
  return for_apply_launches(kind, K, R, w, [&](int k0, int kg, int r0, int rn) {
    return one(kg, rn, k0 > 0, false, dw_pref, k0 == 0 && row_ones && row_ones[r0]);
  });
}

// lsec_test_hold_networks: while set, enqueue_apply takes no compiled network for ready, as on a plan's first calls
std::atomic<int> g_hold_networks{0};
bool networks_held() { return g_hold_networks.load(std::memory_order_relaxed) != 0; }

bool encode_magic_fuses(int kind, int k, int m) {
  return (kind == KBYTEWISE || kind == KBITSLICED) && m <= 8 && k <= lsec::kMaxK && k + m <= lsec::kMaxMagicShards;
}

// Enqueue out[r] = rows[r] . in  for every stripe, splitting R into launches of <= 8 rows
// (<= 2 for the bitmatrix kernel) and K into groups of <= lsec::kMaxK inputs.  `image` is the
// CoefCell[R][K] matrix image, the uint32 row masks [((r*w+l)*K + j)*NW + q] (KBITMATRIX) or the
// word products [(r*K + j)*w + b] (KWORDWISE / KBITSLICEDW), grouped when K > kMaxK.
thread_local int tl_apply_path = 0;  // lsec_test_apply_path: what this thread's last enqueue_apply launched

int enqueue_apply(int kind, const void *image, int K, int R, const ShardRef *in, const ShardRef *out,
                  int nstripes, long long size, int packet, hipStream_t st, int w, const uint8_t *gf8_rows) {
  tl_apply_path = 0;
  const bool net = kind == KBYTEWISE   ? lsec::bytewise_variant() == 0 && lsec::jit::wants_xornet(R, K)
                   : kind == KWORDWISE ? lsec::bitsliced_variant() == 0 && lsec::jit::wants_gfw_net(R, K, w)
                                       : false;
  ShardRef tin[lsec::kMaxK], tout[lsec::kMaxR];  // a w = 16 / 32 network's ragged tail, below
  if (net) {
    if (hipFunction_t fn = networks_held() ? nullptr : lsec::jit::ready(image, R, K)) {  // the matrix's compiled XOR network
      // w = 16 / 32 networks take whole tiles only: the tail columns go to the generic kernel
      const long long whole = kind == KWORDWISE ? size / lsec::jit::gfw_tile(w, R) * lsec::jit::gfw_tile(w, R) : size;
      ShardRef bi[lsec::jit::kMaxCols], bo[lsec::jit::kMaxRows];
      if (whole > 0 && for_launches(nstripes, launch_stripes(size, false), [&](long long s0, int n) {
            for (int j = 0; j < K; ++j) bi[j] = shard_from(in[j], s0);
            for (int r = 0; r < R; ++r) bo[r] = shard_from(out[r], s0);
            const hipError_t err = lsec::jit::launch(fn, R, K, bi, bo, n, whole, st, kind == KWORDWISE ? w : 8);
            if (err != hipSuccess) return fail("xor network launch failed: %s", hipGetErrorString(err));
            tl_apply_path |= 1;
            return 0;
          }))
        return -1;
      if (whole == size) return 0;
      for (int j = 0; j < K; ++j) tin[j] = {in[j].base + static_cast<uint64_t>(whole), in[j].stride};
      for (int r = 0; r < R; ++r) tout[r] = {out[r].base + static_cast<uint64_t>(whole), out[r].stride};
      in = tin;
      out = tout;
      size -= whole;
    }
  }
  // Cauchy w = 8: the shape's kernel (cauchy8_bitsliced_dw; 0 = the network)
  const int c8_dw = apply_dw_pref(kind, K, R, w, size, lsec::bitsliced_variant());
  if ((kind == KBITMATRIX || kind == KBITSLICEDW || kind == KBITSLICED) && lsec::bitsliced_variant() == 0 && c8_dw == 0 &&
      lsec::jit::wants_pktnet(R, K, w) &&
      lsec::jit::pkt_aligned(in, K, out, R, w, packet))
    if (hipFunction_t fn = networks_held() ? nullptr : lsec::jit::ready(image, R, K)) {  // the bitmatrix's compiled packet network
      const hipError_t err = lsec::jit::launch_pkt(fn, R, K, in, out, nstripes, size, packet, w, st);
      if (err != hipSuccess) return fail("packet network launch failed: %s", hipGetErrorString(err));
      tl_apply_path |= 2;
      return 0;
    }
  const int rpr = image_rows_per_output(kind, w), unit = image_unit(kind, w);
  // input groups of at most kMaxK (grouped image layout); groups after the first accumulate
  return for_apply_launches(kind, K, R, w, [&](int k0, int kg, int r0, int rn) {
    const size_t group_base = static_cast<size_t>(k0) * R * rpr * unit;  // earlier groups: kMaxK inputs each
    lsec::ApplyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.K = kg;
    a.R = rn;
    a.accumulate = k0 > 0;
    const size_t at = group_base + static_cast<size_t>(r0) * rpr * kg * unit;
    if (uses_u32_image(kind)) {  // w words per (row, input), or mask words per (bit-row, input)
      a.masks = static_cast<const uint32_t *>(image) + at;
      a.w = w;
    } else {
      a.cells = static_cast<const CoefCell *>(image) + at;
      lsec::apply_record_first_row(apply_first_row_ones(gf8_rows, K, k0, r0));  // (lsec_test_apply_record)
    }
    a.size = size;
    a.packet = packet;
    return for_launches(nstripes, launch_stripes(size, false), [&](long long s0, int n) {
      a.nstripes = n;
      for (int j = 0; j < kg; ++j) a.in[j] = shard_from(in[k0 + j], s0);
      for (int r = 0; r < a.R; ++r) a.out[r] = shard_from(out[r0 + r], s0);
      const hipError_t err = kind == KBYTEWISE     ? lsec::launch_bytewise(a, st)
                             : kind == KBITMATRIX  ? lsec::launch_bitmatrix(a, st)
                             : kind == KWORDWISE   ? lsec::launch_wordwise(a, st)
                             : kind == KBITSLICEDW ? lsec::launch_gfw_bitsliced(a, st)
                                                   : lsec::launch_bitsliced(a, st, 0, c8_dw);
      if (err != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(err));
      tl_apply_path |= 4;
      return 0;
    });
  });
}

// ---------------------------------------------------------------- device-resident core
// a job over device-resident shards: sh[id] for every id of the job
int apply_job(const PlanExt *e, const CodingJob &job, const lsec_shard_t *sh, int nstripes, long long C, hipStream_t st) {
  ShardRef in[kMaxDevs], out[kMaxDevs];
  const int K = static_cast<int>(job.in_ids.size());
  for (int j = 0; j < K; ++j) in[j] = shard_from(sh[job.in_ids[j]], 0);
  for (int r = 0; r < job.R; ++r) out[r] = shard_from(sh[job.out_ids[r]], 0);
  return enqueue_apply(job.kind, job.image, K, job.R, in, out, nstripes, C, e->pub.packet_size, st, e->pub.w, job.gf8_rows);
}

int encode_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, hipStream_t st) {
  if (check_geometry(&e->pub, C)) return -1;
  if (nstripes <= 0 || C == 0) return 0;
  CodingJob job;
  if (encode_job(e, &job)) return -1;
  return apply_job(e, job, sh, nstripes, C, st);
}

// returns 0 (done or nothing to do) / -1
int decode_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, const int *erasures,
               hipStream_t st) {
  lio_erasure_plan_t *p = &e->pub;
  std::vector<int> ids;
  const int pr = parse_erasures(p, erasures, ids);
  if (pr < 0) return -1;
  if (pr == 1) return 0;
  if (check_geometry(p, C)) return -1;
  if (p->method == RAID4 && ids[0] >= p->data_strips) return 0;  // raid4.c:48 leaves lost parity alone
  if (nstripes <= 0 || C == 0) return 0;
  CodingJob job;
  if (decode_job(e, ids, &job)) return -1;
  return apply_job(e, job, sh, nstripes, C, st);
}

// ---------------------------------------------------------------- per-stripe erasure patterns
// lsec_decode_dev_patterns / lsec_decode_dev_rotated: one table of pattern records and matrix
// images (ec_kernels.h, PatRecord) per call shape, built from the per-pattern host plans of
// decode_cache -- the matrices lsec_decode_dev applies -- and cached per device on the plan.

// (first_stripe * n_shift) mod n in 64 bits: first_stripe >= 0, n_shift >= 0, n >= 1
uint32_t pattern_rot0(int n, int n_shift, long long first_stripe) {
  const unsigned long long un = static_cast<unsigned long long>(n);
  return static_cast<uint32_t>((static_cast<unsigned long long>(first_stripe) % un) *
                               (static_cast<unsigned long long>(n_shift) % un) % un);
}

namespace {

int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the limits both calls share; every message names its limit
int pattern_limits(const lio_erasure_plan_t *p) {
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("per-stripe patterns need plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is kernel %d",
                JE_method[p->method], p->w, kind);
  if (p->data_strips < 1 || p->data_strips > lsec::kMaxK)
    return fail("per-stripe patterns: k=%d outside 1..%d", p->data_strips, lsec::kMaxK);
  if (p->parity_strips < 1 || p->data_strips + p->parity_strips > lsec::kPatMaxShards)
    return fail("per-stripe patterns: k+m=%d exceeds %d shards per call", p->data_strips + p->parity_strips,
                lsec::kPatMaxShards);
  return 0;
}

// Appends one pattern's record and image rows to the host table.  `ids`: its erased logical ids
// (sorted, distinct; empty: nothing to rebuild); rot: shard index = (logical id - rot) mod n
// (0 for the patterned call, whose shards are logical chunks).  Takes the plan's mutex.
int pattern_record(PlanExt *e, const std::vector<int> &ids, int rot, lsec::PatRecord &rec, lsec::PatUnused &unused,
                   lsec::gf8::Mat &rows) {
  const lio_erasure_plan_t *p = &e->pub;
  const int k = p->data_strips, n = k + p->parity_strips;
  const auto shard_of = [&](int logical) { return static_cast<uint32_t>(((logical - rot) % n + n) % n); };
  std::memset(&rec, 0, sizeof(rec));
  std::memset(&unused, 0, sizeof(unused));
  rows.clear();
  // What the magic form sums beside the record's inputs and outputs: the logical ids in neither list, ascending.
  // Only tables of m <= 8 have room for them, and only those are ever asked for them (decode_magic_limits).
  const auto note_unused = [&](const std::vector<int> &survivors, const std::vector<int> &erased) {
    if (n - k > lsec::kPatMaxUnused) return;
    for (int c = 0; c < n; ++c)
      if (std::find(survivors.begin(), survivors.end(), c) == survivors.end() &&
          std::find(erased.begin(), erased.end(), c) == erased.end())
        unused.sel[unused.n++] = shard_of(c);
  };
  // nothing to rebuild (raid4.c:48 leaves lost parity alone): the plain kernels leave at nout == 0; the magic
  // form's checksum-only path reads the data chunks as its inputs and the parity as its unused survivors
  if (ids.empty() || (p->method == RAID4 && ids[0] >= k)) {
    std::vector<int> data(k);
    for (int j = 0; j < k; ++j) rec.in_sel[j] = shard_of(data[j] = j);
    note_unused(data, {});
    return 0;
  }
  if (static_cast<int>(ids.size()) > lsec::kPatMaxOut)
    return fail("per-stripe patterns: %zu erasures in one pattern exceed %d", ids.size(), lsec::kPatMaxOut);
  DecodeEntry *ent = nullptr;
  {
    std::lock_guard<std::mutex> lk(e->impl->mu);
    if (decode_host_locked(e, ids, &ent)) return -1;
  }
  // (entries are never moved or freed before the plan is destroyed: decode_entry)
  rec.nout = static_cast<uint32_t>(ent->dp.erased.size());
  for (int j = 0; j < k; ++j) rec.in_sel[j] = shard_of(ent->dp.survivors[j]);
  for (uint32_t r = 0; r < rec.nout; ++r) rec.out_sel[r] = shard_of(ent->dp.erased[r]);
  note_unused(std::vector<int>(ent->dp.survivors.begin(), ent->dp.survivors.begin() + k), ent->dp.erased);
  rows = ent->dp.rows;
  return 0;
}

}  // namespace

// The argument checks of a call shape, and what they yield without any matrix work: the cache key
// and each entry's erased logical ids.  patterns != null: npatterns -1 terminated lists back to
// back; else the rotated call's: entry rot (0 <= rot < n) for every rotation (first_stripe + s) *
// n_shift mod n can take, an empty entry (reachable[rot] = 0) for the others.
struct PatternLists {
  std::vector<int> key;                // PatternTable::key
  std::vector<std::vector<int>> ids;   // erased logical ids per entry (sorted, distinct)
  std::vector<int> rots;               // shard index = (logical id - rot) mod n
  std::vector<char> reachable;
};

int parse_pattern_lists(const lio_erasure_plan_t *p, const int *patterns, int npatterns, const int *lost, int n_shift,
                        PatternLists &pl) {
  if (pattern_limits(p)) return -1;
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  if (patterns) {
    if (npatterns < 1 || npatterns > lsec::kPatMaxPatterns)
      return fail("per-stripe patterns: npatterns=%d outside 1..%d", npatterns, lsec::kPatMaxPatterns);
    pl.key.push_back(0);
    const int *at = patterns;
    for (int i = 0; i < npatterns; ++i) {
      std::vector<int> ids;
      if (parse_erasures(p, at, ids) < 0) return -1;  // id out of range, more than m erasures, ...
      if (static_cast<int>(ids.size()) > lsec::kPatMaxOut)
        return fail("per-stripe patterns: %zu erasures in one pattern exceed %d", ids.size(), lsec::kPatMaxOut);
      while (*at != -1) ++at;
      ++at;
      pl.key.insert(pl.key.end(), ids.begin(), ids.end());
      pl.key.push_back(-1);
      pl.ids.push_back(std::move(ids));
      pl.rots.push_back(0);
      pl.reachable.push_back(1);
    }
    return 0;
  }
  if (!lost) return fail("lost is NULL");
  if (n_shift < 0) return fail("n_shift %d is negative", n_shift);
  std::vector<int> devs;
  for (int i = 0; lost[i] != -1; ++i) {
    if (lost[i] < 0 || lost[i] >= n) return fail("lost device %d out of range 0..%d", lost[i], n - 1);
    if (std::find(devs.begin(), devs.end(), lost[i]) == devs.end()) devs.push_back(lost[i]);
    if (i > 4 * n) return fail("lost list not terminated");
  }
  std::sort(devs.begin(), devs.end());
  if (static_cast<int>(devs.size()) > m) return fail("%zu lost devices exceed m=%d", devs.size(), m);
  if (static_cast<int>(devs.size()) > lsec::kPatMaxOut)
    return fail("per-stripe patterns: %zu lost devices exceed %d", devs.size(), lsec::kPatMaxOut);
  const int step = n_shift % n;
  pl.key.push_back(1);
  pl.key.push_back(step);
  pl.key.insert(pl.key.end(), devs.begin(), devs.end());
  const int g = gcd_int(n, step);  // step 0: n, only rotation 0 occurs
  for (int rot = 0; rot < n; ++rot) {
    std::vector<int> ids;
    const bool occurs = rot % g == 0;
    if (occurs)
      for (int d : devs) ids.push_back((d + rot) % n);
    std::sort(ids.begin(), ids.end());
    pl.ids.push_back(std::move(ids));
    pl.rots.push_back(rot);
    pl.reachable.push_back(occurs ? 1 : 0);
  }
  return 0;
}

// The host table of parsed lists: the matrix work.  No device is touched.
int fill_pattern_table(PlanExt *e, PatternLists &pl, PatternTable &tab) {
  const int k = e->pub.data_strips;
  const std::vector<std::vector<int>> &lists = pl.ids;
  const std::vector<int> &rots = pl.rots;
  tab.key = std::move(pl.key);
  tab.reachable = std::move(pl.reachable);
  if (ensure_coding(e)) return -1;
  const size_t np = lists.size();
  std::vector<lsec::gf8::Mat> rows(np);
  tab.recs.assign(np, lsec::PatRecord());
  tab.unused.assign(np, lsec::PatUnused());
  tab.rmax = 0;
  for (size_t i = 0; i < np; ++i) {
    if (pattern_record(e, lists[i], rots[i], tab.recs[i], tab.unused[i], rows[i])) return -1;
    tab.rmax = std::max(tab.rmax, static_cast<int>(tab.recs[i].nout));
  }
  // each entry's erasure set as a mask of logical ids: what lsec_vote_dev compares a stripe's outside set with
  tab.masks.assign(np, 0);
  for (size_t i = 0; i < np; ++i)
    for (int id : lists[i])
      if (id < 64) tab.masks[i] |= 1ull << id;
  // one CoefCell[rmax][k] image per entry with something to rebuild; rows past its count are zero cells
  tab.cells.clear();
  CoefCell zero;
  lsec::make_cell(0, zero);
  for (size_t i = 0; i < np; ++i) {
    if (tab.recs[i].nout == 0) continue;
    std::vector<CoefCell> h;
    host_cells(rows[i], static_cast<int>(tab.recs[i].nout), k, h);
    tab.recs[i].cells_off = static_cast<uint32_t>(tab.cells.size());
    tab.cells.insert(tab.cells.end(), h.begin(), h.end());
    tab.cells.resize(tab.cells.size() + static_cast<size_t>(tab.rmax - static_cast<int>(tab.recs[i].nout)) * k, zero);
  }
  if (tab.cells.empty()) tab.cells.push_back(zero);  // every entry empty: the kernel reads none of it
  return 0;
}

int build_pattern_table(PlanExt *e, const int *patterns, int npatterns, const int *lost, int n_shift, PatternTable &tab) {
  PatternLists pl;
  if (parse_pattern_lists(&e->pub, patterns, npatterns, lost, n_shift, pl)) return -1;
  return fill_pattern_table(e, pl, tab);
}

namespace {

// the call shape's table on the current device: cached on the plan, built and uploaded once
int pattern_table_dev(PlanExt *e, const int *patterns, int npatterns, const int *lost, int n_shift,
                      const PatternTable **out_tab, PatternTable::Dev *out_dev) {
  PatternLists pl;
  if (parse_pattern_lists(&e->pub, patterns, npatterns, lost, n_shift, pl)) return -1;  // every argument check, before any HIP call
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  const auto on_dev = [&](const PatternTable &tab) {  // both images or neither
    *out_tab = &tab;
    *out_dev = {static_cast<const lsec::PatRecord *>(tab.dev_recs.find(dev)), static_cast<const CoefCell *>(tab.dev_cells.find(dev))};
    return out_dev->cells != nullptr;
  };
  {
    std::lock_guard<std::mutex> lk(e->impl->mu);
    const auto it = e->impl->pattern_cache.find(pl.key);
    if (it != e->impl->pattern_cache.end() && on_dev(it->second)) return 0;  // the repeated call: no matrix work, no upload
  }
  PatternTable fresh;
  if (fill_pattern_table(e, pl, fresh)) return -1;  // (takes the plan's mutex per pattern)
  std::lock_guard<std::mutex> lk(e->impl->mu);
  // (map nodes never move and live until the plan is destroyed, as decode_cache's)
  PatternTable &tab = e->impl->pattern_cache.emplace(fresh.key, std::move(fresh)).first->second;
  if (on_dev(tab)) return 0;
  const void *recs = nullptr, *cells = nullptr;
  if (tab.dev_recs.get(dev, tab.recs.data(), sizeof(lsec::PatRecord) * tab.recs.size(), "hipMemcpy(pattern records)", nullptr, &recs))
    return -1;
  if (tab.dev_cells.get(dev, tab.cells.data(), sizeof(CoefCell) * tab.cells.size(), "hipMemcpy(cells)", nullptr, &cells)) {
    tab.dev_recs.drop(dev);
    return -1;
  }
  on_dev(tab);
  return 0;
}

// the first rotation of the launch that starts at stripe s0
uint32_t rot0_from(uint32_t rot0, uint32_t rot_step, int n, long long s0) {
  return static_cast<uint32_t>((rot0 + (s0 % n) * rot_step) % n);
}

// The launches of a patterned call, split so that tile indices stay 32-bit (as enqueue_apply).  A
// stripe's pattern id comes from stripe_pattern or, without one, from its rotation.  rot_mode:
// kRotSingles, the repair behind a rotated locate, whose table is the k+m single erasures of the
// logical chunks and whose kernel turns each selection into a physical device by the stripe's
// rotation; kRotLogical, the same over any logical table with a stripe_pattern: the repair behind a
// rotated search and lsec_decode_dev_patterns_rotated.
enum { kRotNone = 0, kRotSingles, kRotLogical };
int enqueue_patterns(PlanExt *e, const PatternTable &tab, const PatternTable::Dev &dv, const lsec_shard_t *sh, int nstripes,
                     long long C, const unsigned char *stripe_pattern, uint32_t rot0, uint32_t rot_step, int rot_mode,
                     hipStream_t st) {
  const lio_erasure_plan_t *p = &e->pub;
  const int n = p->data_strips + p->parity_strips;
  if (nstripes <= 0 || C == 0 || tab.rmax == 0) return 0;  // rmax 0: every pattern is empty
  const bool rotates = rot_mode || !stripe_pattern;
  lsec::PatternRotArgs a;  // (PatternArgs, which the type's rotated launches take too)
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.recs = dv.recs;
  a.cells = dv.cells;
  a.npat = static_cast<uint32_t>(tab.recs.size());
  a.K = p->data_strips;
  a.packet = p->packet_size;
  a.nshards = n;
  a.size = C;
  a.rot_step = rot_step;
  a.rot_n = rotates ? static_cast<uint32_t>(n) : 0;
  // a Cauchy plan's patterns all take the bit-sliced kernel, 0 / 1 rows too (the same bytes in either layout)
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  return for_launches(nstripes, launch_stripes(C, true), [&](long long s0, int ns) {
    a.nstripes = ns;
    for (int i = 0; i < n; ++i) a.sh[i] = shard_from(sh[i], s0);
    a.stripe_pattern = stripe_pattern ? stripe_pattern + s0 : nullptr;
    a.rot0 = rotates ? rot0_from(rot0, rot_step, n, s0) : 0;
    if (rot_mode == kRotLogical) {
      const hipError_t err = sliced ? lsec::launch_pattern_rot_rows_bitsliced(a, tab.rmax, st) : lsec::launch_pattern_rot_rows_bytewise(a, tab.rmax, st);
      if (err != hipSuccess) return fail("rotated pattern kernel launch failed: %s", hipGetErrorString(err));
    } else if (rot_mode) {
      const hipError_t err = sliced ? lsec::launch_pattern_rot_bitsliced(a, st) : lsec::launch_pattern_rot_bytewise(a, st);
      if (err != hipSuccess) return fail("rotated repair kernel launch failed: %s", hipGetErrorString(err));
    } else {
      const hipError_t err = sliced ? lsec::launch_pattern_bitsliced(a, tab.rmax, st) : lsec::launch_pattern_bytewise(a, tab.rmax, st);
      if (err != hipSuccess) return fail("pattern kernel launch failed: %s", hipGetErrorString(err));
    }
    return 0;
  });
}

// The rungs the calls with a pattern list and a stripe_pattern share, in their order (the rotation's two only for a
// call over rotated devices); the message is the caller's to name.
int patterns_call_args(const lio_erasure_plan_t *p, const PatternRot *rot, int nstripes, long long C, const int *patterns,
                       const unsigned char *stripe_pattern) {
  if (!patterns) return fail("patterns is NULL");
  if (nstripes < 0) return fail("nstripes %d is negative", nstripes);
  if (rot && rot->n_shift < 0) return fail("n_shift %d is negative", rot->n_shift);
  if (rot && rot->first_stripe < 0) return fail("first_stripe %lld is negative", rot->first_stripe);
  if (nstripes > 0 && !stripe_pattern) return fail("stripe_pattern is NULL");
  if (pattern_limits(p) || check_geometry(p, C)) return -1;
  return 0;
}

}  // namespace

// lsec_decode_dev_patterns (rot null, name null: its messages stand as they are) and lsec_decode_dev_patterns_rotated:
// one path, the rotation a parameter.  Rotated, the launches are the k_patrot_* kernels of the table's row count over
// the same logical table, which is what the repair behind a rotated search runs.
int decode_dev_patterns(PlanExt *e, const char *name, const PatternRot *rot, const lsec_shard_t *sh, int nstripes, long long C,
                        const int *patterns, int npatterns, const unsigned char *stripe_pattern, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  if (named(name, patterns_call_args(p, rot, nstripes, C, patterns, stripe_pattern))) return -1;
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  if (named(name, pattern_table_dev(e, patterns, npatterns, nullptr, 0, &tab, &dv))) return -1;
  const int n = p->data_strips + p->parity_strips;
  const uint32_t rot0 = rot ? pattern_rot0(n, rot->n_shift, rot->first_stripe) : 0;
  const uint32_t rot_step = rot ? static_cast<uint32_t>(rot->n_shift % n) : 0;
  return named(name, enqueue_patterns(e, *tab, dv, sh, nstripes, C, stripe_pattern, rot0, rot_step, rot ? kRotLogical : kRotNone, st));
}

int decode_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, const int *lost, int n_shift,
                       long long first_stripe, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  if (!lost) return fail("lost is NULL");
  if (nstripes < 0) return fail("nstripes %d is negative", nstripes);
  if (n_shift < 0) return fail("n_shift %d is negative", n_shift);
  if (first_stripe < 0) return fail("first_stripe %lld is negative", first_stripe);
  if (pattern_limits(p) || check_geometry(p, C)) return -1;
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  if (pattern_table_dev(e, nullptr, 0, lost, n_shift, &tab, &dv)) return -1;
  const int n = p->data_strips + p->parity_strips;
  return enqueue_patterns(e, *tab, dv, devs, nstripes, C, nullptr, pattern_rot0(n, n_shift, first_stripe),
                          static_cast<uint32_t>(n_shift % n), kRotNone, st);
}

// ---------------------------------------------------------------- patterned decode with the stripe magics
// lsec_decode_magic_dev_patterns / _rotated / _patterns_rotated: the plain calls' table, launches and split, with the MG
// kernels (ec_kernels.h, PatternMagicArgs) over 16 bytes per stripe of accumulators from the
// stream-ordered allocator -- zeroed before the first launch, advancing by 2 * s0 words per launch,
// freed on the stream -- and one finalize launch behind the tile launches.  The table is the plain
// calls' own cache entry; the unused-survivor records it carries are uploaded at the first magic call
// on a device and cached with it.  Every refusal names the call; all of them come before the first
// HIP call.
int named(const char *name, int rc) {
  if (rc && name) {
    const std::string why = tl_err;  // the shared rule's message, behind the call's name
    fail("%s: %s", name, why.c_str());
  }
  return rc;
}

int decode_magic_limits(const lio_erasure_plan_t *p, const char *name) {
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", name,
                JE_method[p->method], p->w, kind);
  if (p->data_strips < 1 || p->data_strips > lsec::kMaxK)
    return fail("%s: k=%d outside 1..%d", name, p->data_strips, lsec::kMaxK);
  if (p->parity_strips < 1 || p->parity_strips > lsec::kPatMaxUnused)
    return fail("%s: m=%d outside 1..%d (the survivors a pattern's decode does not read, and the 32-bit lane sums)", name,
                p->parity_strips, lsec::kPatMaxUnused);
  return 0;
}

namespace {

int magic_check_args(const char *name, const MagicCheck &mc, int nstripes) {
  if (nstripes > 0 && !mc.magic) return fail("%s: magic is NULL", name);
  if (mc.bad && !mc.expect) return fail("%s: bad is given without expect (there is nothing to compare with)", name);
  if (mc.bad_count && !mc.expect) return fail("%s: bad_count is given without expect (there is nothing to compare with)", name);
  if (reinterpret_cast<uintptr_t>(mc.bad_count) % 4 != 0)
    return fail("%s: bad_count %p is not a multiple of 4 bytes (one 32-bit word)", name, static_cast<const void *>(mc.bad_count));
  return 0;
}

// the table's unused-survivor records on the current device: uploaded once, cached with the table
int pattern_unused_dev(PlanExt *e, const PatternTable *ctab, const lsec::PatUnused **out) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(e->impl->mu);
  PatternTable &tab = *const_cast<PatternTable *>(ctab);  // (a node of the plan's own map, guarded by its mutex)
  const void *p = tab.dev_unused.find(dev);
  if (!p && tab.dev_unused.get(dev, tab.unused.data(), sizeof(lsec::PatUnused) * tab.unused.size(),
                               "hipMemcpy(unused survivors)", nullptr, &p))
    return -1;
  *out = static_cast<const lsec::PatUnused *>(p);
  return 0;
}

// enqueue_patterns for the MG kernels.  A table whose patterns are all empty still launches (one row:
// its tiles only checksum).  rot_logical: the shards are the devices of a rotated LUN and the table is
// a logical one with a stripe_pattern (the k_patmagicrot_* kernels); without a stripe_pattern the
// table's own records rotate (k_patmagic_*), as in enqueue_patterns.
int enqueue_patterns_magic(PlanExt *e, const char *name, const PatternTable &tab, const PatternTable::Dev &dv,
                           const lsec::PatUnused *unused, const lsec_shard_t *sh, int nstripes, long long C,
                           const unsigned char *stripe_pattern, uint32_t rot0, uint32_t rot_step, bool rot_logical,
                           const MagicCheck &mc, hipStream_t st) {
  const lio_erasure_plan_t *p = &e->pub;
  const int n = p->data_strips + p->parity_strips;
  if (nstripes <= 0) return 0;
  if (rot_logical && !stripe_pattern) return fail("%s: a rotated logical table needs a stripe_pattern", name);
  const bool rotates = rot_logical || !stripe_pattern;  // (rot_n stays 0 otherwise: nothing divides by it)
  const int rmax = std::max(1, tab.rmax);
  lsec::PatternMagicRotArgs a;  // (PatternMagicArgs, which the other launches take)
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.recs = dv.recs;
  a.cells = dv.cells;
  a.unused = unused;
  a.npat = static_cast<uint32_t>(tab.recs.size());
  a.K = p->data_strips;
  a.packet = p->packet_size;
  a.nshards = n;
  a.size = C;
  a.rot_step = rot_step;
  a.rot_n = rotates ? static_cast<uint32_t>(n) : 0;
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  unsigned long long *acc = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&acc), 16ull * nstripes, st);
  if (err == hipSuccess && (err = hipMemsetAsync(acc, 0, 16ull * nstripes, st)) != hipSuccess) (void)hipFreeAsync(acc, st);
  if (err != hipSuccess) return fail("%s: the magic accumulators (%llu bytes): %s", name, 16ull * nstripes, hipGetErrorString(err));
  int rc = 0;
  if (mc.bad_count && (err = hipMemsetAsync(mc.bad_count, 0, sizeof(unsigned), st)) != hipSuccess)
    rc = fail("%s: zeroing bad_count: %s", name, hipGetErrorString(err));
  if (rc == 0)
    rc = for_launches(nstripes, launch_stripes(C, true), [&](long long s0, int ns) {
      a.nstripes = ns;
      for (int i = 0; i < n; ++i) a.sh[i] = shard_from(sh[i], s0);
      a.stripe_pattern = stripe_pattern ? stripe_pattern + s0 : nullptr;
      a.rot0 = rotates ? rot0_from(rot0, rot_step, n, s0) : 0;
      a.magic_acc = acc + 2 * s0;
      hipError_t le;
      if (rot_logical) le = sliced ? lsec::launch_pattern_magic_rot_bitsliced(a, rmax, st) : lsec::launch_pattern_magic_rot_bytewise(a, rmax, st);
      else le = sliced ? lsec::launch_pattern_magic_bitsliced(a, rmax, st) : lsec::launch_pattern_magic_bytewise(a, rmax, st);
      if (le != hipSuccess) return fail("%s: kernel launch failed: %s", name, hipGetErrorString(le));
      return 0;
    });
  if (rc == 0) {
    err = lsec::launch_pattern_magic_finalize(acc, stripe_pattern, a.npat, nstripes, static_cast<int64_t>(n) * C, mc.magic,
                                              mc.expect, mc.bad, mc.bad_count, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", name, hipGetErrorString(err));
  }
  err = hipFreeAsync(acc, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the magic accumulators: %s", name, hipGetErrorString(err));
  return rc;
}

}  // namespace

// lsec_decode_magic_dev_patterns (rot null) and lsec_decode_magic_dev_patterns_rotated: one path, the rotation a
// parameter.
int decode_magic_dev_patterns(PlanExt *e, const char *name, const PatternRot *rot, const lsec_shard_t *sh, int nstripes,
                              long long C, const int *patterns, int npatterns, const unsigned char *stripe_pattern,
                              const MagicCheck &mc, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  if (named(name, patterns_call_args(p, rot, nstripes, C, patterns, stripe_pattern))) return -1;
  {
    PatternLists pl;  // the lists' own refusals, ahead of the magic's (pattern_table_dev parses them again)
    if (named(name, parse_pattern_lists(p, patterns, npatterns, nullptr, 0, pl))) return -1;
  }
  if (magic_check_args(name, mc, nstripes)) return -1;
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  const lsec::PatUnused *unused = nullptr;
  if (named(name, pattern_table_dev(e, patterns, npatterns, nullptr, 0, &tab, &dv)) || named(name, pattern_unused_dev(e, tab, &unused)))
    return -1;
  const int n = p->data_strips + p->parity_strips;
  const uint32_t rot0 = rot ? pattern_rot0(n, rot->n_shift, rot->first_stripe) : 0;
  const uint32_t rot_step = rot ? static_cast<uint32_t>(rot->n_shift % n) : 0;
  return enqueue_patterns_magic(e, name, *tab, dv, unused, sh, nstripes, C, stripe_pattern, rot0, rot_step, rot != nullptr, mc, st);
}

int decode_magic_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, const int *lost, int n_shift,
                             long long first_stripe, const MagicCheck &mc, hipStream_t st) {
  static const char name[] = "lsec_decode_magic_dev_rotated";
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  if (!lost) return fail("%s: lost is NULL", name);
  if (nstripes < 0) return fail("%s: nstripes %d is negative", name, nstripes);
  if (n_shift < 0) return fail("%s: n_shift %d is negative", name, n_shift);
  if (first_stripe < 0) return fail("%s: first_stripe %lld is negative", name, first_stripe);
  if (named(name, pattern_limits(p) || check_geometry(p, C) ? -1 : 0)) return -1;
  {
    PatternLists pl;
    if (named(name, parse_pattern_lists(p, nullptr, 0, lost, n_shift, pl))) return -1;
  }
  if (magic_check_args(name, mc, nstripes)) return -1;
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  const lsec::PatUnused *unused = nullptr;
  if (named(name, pattern_table_dev(e, nullptr, 0, lost, n_shift, &tab, &dv)) || named(name, pattern_unused_dev(e, tab, &unused)))
    return -1;
  const int n = p->data_strips + p->parity_strips;
  return enqueue_patterns_magic(e, name, *tab, dv, unused, devs, nstripes, C, nullptr, pattern_rot0(n, n_shift, first_stripe),
                                static_cast<uint32_t>(n_shift % n), false, mc, st);
}

// ---------------------------------------------------------------- the search for the erasure set that fits the magic
// lsec_search_dev_patterns / _rotated: jerase_brute_recovery (segment/jerasure.c:271-339) over device-resident
// stripes.  The table is the cache entry lsec_decode_dev_patterns uses for the same list, with the magic
// form's unused-survivor records, so the search, the repair and a later decode with `found` share one
// upload.  The SR kernels (ec_kernels.h, PatternSearchArgs) try every candidate on every selected stripe
// over 16 bytes per (stripe, candidate) of accumulators from the stream-ordered allocator -- zeroed before
// the first launch, advancing by 2 * s0 * npatterns words per launch, freed on the stream, also when a
// launch fails -- and one finalize launch behind them writes trial and found and counts.  A launch takes
// whole stripes with all their candidates: the split counts (stripe, candidate) pairs, and
// lsec_test_set_pattern_split lowers it.  With LSEC_SEARCH_REPAIR the patterned decode follows on the
// stream with found as its stripe_pattern (rotated: the k_patrot_* kernels of the table's row count).
// Every refusal names the call; all of them come before the first HIP call.
// The form that ships is the better measured one (profiles/search_ab.jsonl): the candidate innermost
// in the tile order, plain loads.  lsec_test_set_search_form picks another for A/B runs.
std::atomic<int> g_search_cand_outer{0}, g_search_plain_loads{1};

namespace {

struct SearchCall {
  const char *name;
  bool rotated;
  int n_shift;
  long long first_stripe;
  const uint8_t *select;
  const uint8_t *expect;
  uint8_t *found;
  uint8_t *trial;
  unsigned *counts;
  int flags;
};

constexpr int kSearchMaxPatterns = 254;  // LSEC_LOCATE_MANY and LSEC_LOCATE_CLEAN stay past the table

// stripes per launch: every stripe brings npat candidates' tiles
long long search_launch_stripes(long long C, int npat) { return std::max(1LL, launch_stripes(C, false) / npat); }

int search_dev(PlanExt *e, const SearchCall &c, const lsec_shard_t *sh, int nstripes, long long C, const int *patterns,
               int npatterns, hipStream_t st) {
  const char *name = c.name;
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  if (!patterns) return fail("%s: patterns is NULL", name);
  if (nstripes < 0) return fail("%s: nstripes %d is negative", name, nstripes);
  if (c.rotated && c.n_shift < 0) return fail("%s: n_shift %d is negative", name, c.n_shift);
  if (c.rotated && c.first_stripe < 0) return fail("%s: first_stripe %lld is negative", name, c.first_stripe);
  if (named(name, pattern_limits(p) || check_geometry(p, C) ? -1 : 0)) return -1;
  {
    PatternLists pl;  // the lists' own refusals, ahead of the search's (pattern_table_dev parses them again)
    if (named(name, parse_pattern_lists(p, patterns, npatterns, nullptr, 0, pl))) return -1;
  }
  if (npatterns > kSearchMaxPatterns)
    return fail("%s: npatterns=%d outside 1..%d (found[] keeps LSEC_LOCATE_MANY and LSEC_LOCATE_CLEAN past the table)", name,
                npatterns, kSearchMaxPatterns);
  if (static_cast<long long>(nstripes) * npatterns >= (1LL << 31))
    return fail("%s: nstripes * npatterns = %lld is not below 2^31 (stripe, candidate) pairs per call", name,
                static_cast<long long>(nstripes) * npatterns);
  if (nstripes > 0 && !c.expect) return fail("%s: expect is NULL", name);
  if (nstripes > 0 && !c.found) return fail("%s: found is NULL", name);
  if (reinterpret_cast<uintptr_t>(c.counts) % 4 != 0)
    return fail("%s: counts %p is not a multiple of 4 bytes (two 32-bit words)", name, static_cast<const void *>(c.counts));
  if (c.flags & ~LSEC_SEARCH_REPAIR) return fail("%s: unknown flags 0x%x (LSEC_SEARCH_REPAIR = 1 is the only one)", name, c.flags);
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  const lsec::PatUnused *unused = nullptr;
  if (named(name, pattern_table_dev(e, patterns, npatterns, nullptr, 0, &tab, &dv)) || named(name, pattern_unused_dev(e, tab, &unused)))
    return -1;
  if (nstripes <= 0) return 0;

  const int n = p->data_strips + p->parity_strips;
  const int rmax = std::max(1, tab->rmax);
  const uint32_t rot_step = c.rotated ? static_cast<uint32_t>(c.n_shift % n) : 0;
  const uint32_t rot0 = c.rotated ? pattern_rot0(n, c.n_shift, c.first_stripe) : 0;
  lsec::PatternSearchRotArgs a;  // (PatternSearchArgs, which the unrotated launches take)
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.recs = dv.recs;
  a.cells = dv.cells;
  a.unused = unused;
  a.npat = static_cast<uint32_t>(npatterns);
  a.K = p->data_strips;
  a.packet = p->packet_size;
  a.nshards = n;
  a.size = C;
  a.rot_step = rot_step;
  a.rot_n = c.rotated ? static_cast<uint32_t>(n) : 0;
  a.cand_outer = g_search_cand_outer.load(std::memory_order_relaxed) ? 1 : 0;
  a.plain_loads = g_search_plain_loads.load(std::memory_order_relaxed) ? 1 : 0;
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  const unsigned long long acc_bytes = 16ull * nstripes * npatterns;
  unsigned long long *acc = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&acc), acc_bytes, st);
  if (err == hipSuccess && (err = hipMemsetAsync(acc, 0, acc_bytes, st)) != hipSuccess) (void)hipFreeAsync(acc, st);
  if (err != hipSuccess) return fail("%s: the magic accumulators (%llu bytes): %s", name, acc_bytes, hipGetErrorString(err));
  int rc = 0;
  if (c.counts && (err = hipMemsetAsync(c.counts, 0, 2 * sizeof(unsigned), st)) != hipSuccess)
    rc = fail("%s: zeroing counts: %s", name, hipGetErrorString(err));
  long long per = search_launch_stripes(C, npatterns);
  if (const int hook = g_pattern_split.load(std::memory_order_relaxed); hook > 0) per = std::min<long long>(per, hook);
  if (rc == 0)
    rc = for_launches(nstripes, per, [&](long long s0, int ns) {
      a.nstripes = ns;
      for (int i = 0; i < n; ++i) a.sh[i] = shard_from(sh[i], s0);
      a.select = c.select ? c.select + s0 : nullptr;
      a.rot0 = c.rotated ? rot0_from(rot0, rot_step, n, s0) : 0;
      a.magic_acc = acc + 2 * s0 * npatterns;
      hipError_t le;
      if (c.rotated) le = sliced ? lsec::launch_pattern_search_bitsliced(a, rmax, st) : lsec::launch_pattern_search_bytewise(a, rmax, st);
      else {
        const lsec::PatternSearchArgs &u = a;
        le = sliced ? lsec::launch_pattern_search_bitsliced(u, rmax, st) : lsec::launch_pattern_search_bytewise(u, rmax, st);
      }
      if (le != hipSuccess) return fail("%s: kernel launch failed: %s", name, hipGetErrorString(le));
      return 0;
    });
  if (rc == 0) {
    err = lsec::launch_pattern_search_finalize(acc, c.select, a.npat, nstripes, static_cast<int64_t>(n) * C, c.expect, c.found,
                                               c.trial, c.counts, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", name, hipGetErrorString(err));
  }
  err = hipFreeAsync(acc, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the magic accumulators: %s", name, hipGetErrorString(err));
  if (rc || !(c.flags & LSEC_SEARCH_REPAIR)) return rc;
  // every found stripe rebuilt in place: found[s] < npatterns names its pattern, both sentinels leave a stripe alone
  return named(name, enqueue_patterns(e, *tab, dv, sh, nstripes, C, c.found, rot0, rot_step, c.rotated ? kRotLogical : kRotNone, st));
}

}  // namespace

int search_dev_patterns(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, const int *patterns, int npatterns,
                        const uint8_t *select, const uint8_t *expect, uint8_t *found, uint8_t *trial, unsigned *counts, int flags,
                        hipStream_t st) {
  const SearchCall c = {"lsec_search_dev_patterns", false, 0, 0, select, expect, found, trial, counts, flags};
  return search_dev(e, c, sh, nstripes, C, patterns, npatterns, st);
}

int search_dev_patterns_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                                const int *patterns, int npatterns, const uint8_t *select, const uint8_t *expect, uint8_t *found,
                                uint8_t *trial, unsigned *counts, int flags, hipStream_t st) {
  const SearchCall c = {"lsec_search_dev_patterns_rotated", true, n_shift, first_stripe, select, expect, found, trial, counts, flags};
  return search_dev(e, c, devs, nstripes, C, patterns, npatterns, st);
}

// ---------------------------------------------------------------- the quorum vote over the stored magics
// lsec_vote_dev / _rotated: the first step of segjerase_read_func (segment/jerasure.c:1383-1462) over device-resident
// magics and chunks, so that the quorum and stripe_pattern arrays the calls above take are made where they are used.
// Three launches (ec_vote.h) over 16 bytes per stripe of scratch from the stream-ordered allocator -- zeroed there and
// freed there, also when a launch fails: the vote of the whole call, the blank scan in ranges of stripes whose tile
// indices stay 32-bit (lsec_test_set_pattern_split lowers them; skipped without chunks), and the finalize.  The list's
// masks are one more member of the cache entry lsec_decode_dev_patterns uses for the same list (PatternTable::masks),
// uploaded at the first vote on a device.  Every refusal names the call; all of them come before the first HIP call.
// The scan's form that ships is the best measured one (profiles/vote_ab.jsonl): non-temporal loads,
// tiles of two 16-byte steps per lane;
// lsec_test_set_vote_form picks another for A/B runs.
std::atomic<int> g_vote_plain_loads{0}, g_vote_steps{2};

namespace {

struct VoteCall {
  const char *name;
  bool rotated;
  int n_shift;
  long long first_stripe;
};

// the table's erasure masks on the current device: uploaded once, cached with the table
int pattern_masks_dev(PlanExt *e, const PatternTable *ctab, const unsigned long long **out) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(e->impl->mu);
  PatternTable &tab = *const_cast<PatternTable *>(ctab);  // (a node of the plan's own map, guarded by its mutex)
  const void *p = tab.dev_masks.find(dev);
  if (!p && tab.dev_masks.get(dev, tab.masks.data(), sizeof(unsigned long long) * tab.masks.size(), "hipMemcpy(pattern masks)",
                              nullptr, &p))
    return -1;
  *out = static_cast<const unsigned long long *>(p);
  return 0;
}

int vote_path(PlanExt *e, const VoteCall &c, const lsec_shard_t *stored, const lsec_shard_t *sh, int nstripes, long long C,
              const int *patterns, int npatterns, const VoteOut &o, int flags, hipStream_t st) {
  const char *name = c.name;
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", name,
                JE_method[p->method], p->w, kind);
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  if (k < 1 || k > lsec::kMaxK) return fail("%s: k=%d outside 1..%d", name, k, lsec::kMaxK);
  if (m < 1 || m > 8) return fail("%s: m=%d outside 1..8", name, m);
  if (n > lsec::kVoteMaxShards)
    return fail("%s: k+m=%d exceeds %d (one bit of the outside mask and one lane of the wave per chunk)", name, n, lsec::kVoteMaxShards);
  if (!stored) return fail("%s: stored is NULL", name);
  if (nstripes < 0) return fail("%s: nstripes %d is negative", name, nstripes);
  if (c.rotated && c.n_shift < 0) return fail("%s: n_shift %d is negative", name, c.n_shift);
  if (c.rotated && c.first_stripe < 0) return fail("%s: first_stripe %lld is negative", name, c.first_stripe);
  if (patterns) {
    PatternLists pl;  // the lists' own refusals (pattern_table_dev parses them again)
    if (named(name, parse_pattern_lists(p, patterns, npatterns, nullptr, 0, pl))) return -1;
    if (npatterns > kSearchMaxPatterns)
      return fail("%s: npatterns=%d outside 1..%d (ids[] keeps LSEC_LOCATE_MANY and LSEC_LOCATE_CLEAN past the table)", name,
                  npatterns, kSearchMaxPatterns);
  }
  if (o.ids && !patterns) return fail("%s: ids is given without patterns (there is no list to look the outside set up in)", name);
  if (sh) {
    // lsec_check_dev's rule for every chunk the scan can read: an entry whose stored base is NULL is never read
    for (int i = 0; i < n; ++i) {
      if (!stored[i].base) continue;
      if (reinterpret_cast<uintptr_t>(sh[i].base) % 8 != 0)
        return fail("%s: shard %d: base %p is not a multiple of 8 bytes (lsec_shard_t)", name, i, sh[i].base);
      if (nstripes > 1 && sh[i].stride % 8 != 0)
        return fail("%s: shard %d: stride %lld is not a multiple of 8 bytes (lsec_shard_t)", name, i, sh[i].stride);
    }
    if (named(name, check_geometry(p, C))) return -1;
  }
  if (nstripes > 0 && !o.quorum) return fail("%s: quorum is NULL (4 bytes per stripe, required with nstripes > 0)", name);
  if (nstripes > 0 && !o.cls) return fail("%s: cls is NULL (1 byte per stripe, required with nstripes > 0)", name);
  if (reinterpret_cast<uintptr_t>(o.outside) % 8 != 0)
    return fail("%s: outside %p is not a multiple of 8 bytes (64-bit words)", name, static_cast<const void *>(o.outside));
  if (reinterpret_cast<uintptr_t>(o.counts) % 4 != 0)
    return fail("%s: counts %p is not a multiple of 4 bytes (five 32-bit words)", name, static_cast<const void *>(o.counts));
  if (flags & ~LSEC_VOTE_PARANOID) return fail("%s: unknown flags 0x%x (LSEC_VOTE_PARANOID = 1 is the only one)", name, flags);
  const unsigned long long *masks = nullptr;
  if (patterns) {
    const PatternTable *tab = nullptr;
    PatternTable::Dev dv;
    if (named(name, pattern_table_dev(e, patterns, npatterns, nullptr, 0, &tab, &dv)) || named(name, pattern_masks_dev(e, tab, &masks)))
      return -1;
  }
  if (nstripes <= 0) return 0;

  const unsigned long long scratch_bytes = sizeof(lsec::VoteScratch) * static_cast<unsigned long long>(nstripes);
  lsec::VoteScratch *scratch = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&scratch), scratch_bytes, st);
  if (err == hipSuccess && (err = hipMemsetAsync(scratch, 0, scratch_bytes, st)) != hipSuccess) (void)hipFreeAsync(scratch, st);
  if (err != hipSuccess) return fail("%s: the vote's scratch (%llu bytes): %s", name, scratch_bytes, hipGetErrorString(err));
  int rc = 0;
  if (o.counts && (err = hipMemsetAsync(o.counts, 0, 5 * sizeof(unsigned), st)) != hipSuccess)
    rc = fail("%s: zeroing counts: %s", name, hipGetErrorString(err));
  const bool scans = sh != nullptr && C > 0;
  if (rc == 0) {
    lsec::VoteArgs a;
    std::memset(static_cast<void *>(&a), 0, sizeof(a));
    a.masks = masks;
    a.npat = patterns ? static_cast<uint32_t>(npatterns) : 0;
    a.rot_n = c.rotated ? static_cast<uint32_t>(n) : 0;
    a.rot_step = c.rotated ? static_cast<uint32_t>(c.n_shift % n) : 0;
    a.rot0 = c.rotated ? pattern_rot0(n, c.n_shift, c.first_stripe) : 0;
    a.n = n;
    a.K = k;
    a.nstripes = nstripes;
    a.scan = sh != nullptr;  // (chunks of no bytes are all zero: such a candidate stays blank)
    a.quorum = o.quorum;
    a.outside = o.outside;
    a.scratch = scratch;
    for (int i = 0; i < n; ++i) a.stored[i] = {reinterpret_cast<uint64_t>(stored[i].base), stored[i].stride};
    err = lsec::launch_vote(a, st);
    if (err != hipSuccess) rc = fail("%s: vote kernel launch failed: %s", name, hipGetErrorString(err));
  }
  if (rc == 0 && scans) {
    const int steps = g_vote_steps.load(std::memory_order_relaxed), plain = g_vote_plain_loads.load(std::memory_order_relaxed);
    lsec::VoteScanArgs a;
    std::memset(static_cast<void *>(&a), 0, sizeof(a));
    a.n = n;
    a.size = C;
    long long per = std::max(1LL, launch_stripes(C, false, lsec::vote_scan_tile_bytes(steps)) / n);
    if (const int hook = g_pattern_split.load(std::memory_order_relaxed); hook > 0) per = std::min<long long>(per, hook);
    rc = for_launches(nstripes, per, [&](long long s0, int ns) {
      a.nstripes = ns;
      a.scratch = scratch + s0;
      // (an entry whose stored base is NULL keeps a zero ref: no stripe of the call is a candidate then)
      for (int i = 0; i < n; ++i) a.sh[i] = stored[i].base ? shard_from(sh[i], s0) : ShardRef{0, 0};
      const hipError_t le = lsec::launch_vote_scan(a, plain, steps, st);
      if (le != hipSuccess) return fail("%s: blank scan kernel launch failed: %s", name, hipGetErrorString(le));
      return 0;
    });
  }
  if (rc == 0) {
    err = lsec::launch_vote_finalize(scratch, nstripes, (flags & LSEC_VOTE_PARANOID) ? 1 : 0, patterns ? 1 : 0, o.cls, o.ids, o.counts, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", name, hipGetErrorString(err));
  }
  err = hipFreeAsync(scratch, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the vote's scratch: %s", name, hipGetErrorString(err));
  return rc;
}

}  // namespace

int vote_dev(PlanExt *e, const lsec_shard_t *stored, const lsec_shard_t *sh, int nstripes, long long C, const int *patterns,
             int npatterns, const VoteOut &out, int flags, hipStream_t st) {
  const VoteCall c = {"lsec_vote_dev", false, 0, 0};
  return vote_path(e, c, stored, sh, nstripes, C, patterns, npatterns, out, flags, st);
}

int vote_dev_rotated(PlanExt *e, const lsec_shard_t *stored, const lsec_shard_t *devs, int nstripes, long long C, int n_shift,
                     long long first_stripe, const int *patterns, int npatterns, const VoteOut &out, int flags, hipStream_t st) {
  const VoteCall c = {"lsec_vote_dev_rotated", true, n_shift, first_stripe};
  return vote_path(e, c, stored, devs, nstripes, C, patterns, npatterns, out, flags, st);
}

// ---------------------------------------------------------------- check / locate, rotated or not
// lsec_check_dev: syndrome[s] bit r = parity row r of stripe s, as encode_dev would write it,
// differs from the stored one.  One launch per 32-bit range of tiles (as enqueue_apply) over the
// encode image, in the encode's launch shape; the words are zeroed on the stream ahead of it.
//
// lsec_locate_dev: the check's pass, whose differences S_r are the stripe's syndromes.  A wrong
// data chunk j shows as S_r = Q[r-1][j] * S_0 at every byte column, Q[r-1][j] = g[r][j] / g[0][j]
// (the ratio image, cached on the plan per device as the encode image is); a wrong parity chunk r
// as S_r alone.  The accumulate launches OR row masks into syndrome and AND hypothesis masks into
// hyp, both set on the stream ahead of them; one finalize launch behind them writes located and
// counts.  With LSEC_LOCATE_REPAIR the patterned decode follows on the stream over the k+m
// single-erasure table, located as its stripe_pattern.
//
// lsec_check_dev_rotated / lsec_locate_dev_rotated: the same over the k+m physical devices of a
// rotated LUN.  The kernels work each stripe's rotation out themselves (ec_kernels.h, CheckRotArgs),
// so the outputs are those of the logical view; the finalize launch also names the device behind
// each located chunk.  Each later launch's rot0 advances by (s0 mod n) * rot_step.
//
// lsec_check_magic_dev / lsec_check_magic_dev_rotated: the check's pass with the MG kernels
// (ec_kernels.h, CheckMagicArgs), which also sum each stripe's adler32 magic from the chunks the check
// holds in registers, over 16 bytes per stripe of accumulators from the stream-ordered allocator --
// zeroed before the first launch, advancing by 2 * s0 words per launch, freed on the stream -- and one
// finalize launch behind the tile launches that writes the magic words, compares them with expect,
// writes bad and counts.  The tile launches get no bad_count.  Their rungs sit behind the check's, and
// every message of theirs carries the call's name.
//
// The six calls are one path (scrub_dev) that a ScrubCall steers.

// The host ratio image.  The hypothesis test divides by g[0][j] and tells "row r untouched" from
// "row r touched" by g[r][j] != 0, so a zero coefficient anywhere is refused.
int locate_ratio(PlanExt *e, const lsec::gf8::Mat **out) {
  if (ensure_coding(e)) return -1;
  std::lock_guard<std::mutex> lk(e->impl->mu);
  const int k = e->pub.data_strips, m = e->pub.parity_strips;
  if (e->impl->ratio.empty()) {
    const lsec::gf8::Mat &g = e->impl->coding;
    if (static_cast<int>(g.size()) != m * k) return fail("lsec_locate_dev: the plan encodes %zu parity rows, m=%d", g.size() / k, m);
    lsec::gf8::Mat q(static_cast<size_t>(m - 1) * k);
    for (int r = 0; r < m; ++r)
      for (int j = 0; j < k; ++j) {
        if (g[static_cast<size_t>(r) * k + j] == 0)
          return fail("lsec_locate_dev: coding matrix coefficient [%d][%d] is zero: a data chunk that leaves a parity row "
                      "untouched cannot be told from that row's own corruption", r, j);
        if (r > 0) q[static_cast<size_t>(r - 1) * k + j] = lsec::gf8::div(g[static_cast<size_t>(r) * k + j], g[j]);
      }
    e->impl->ratio = std::move(q);
  }
  *out = &e->impl->ratio;
  return 0;
}

namespace {

// the ratio image on the current device: built and uploaded once per plan and device
int ratio_cells_dev(PlanExt *e, const CoefCell **out) {
  const lsec::gf8::Mat *q = nullptr;
  if (locate_ratio(e, &q)) return -1;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(e->impl->mu);
  static const std::vector<uint32_t> none;
  const CoefSource src = {KNONE, false, false, *q, none, none, e->pub.parity_strips - 1, e->pub.data_strips};  // (k <= kMaxK: one group)
  const void *d = nullptr;
  if (coef_image(e, e->impl->ratio_image, dev, src, &d)) return -1;
  *out = static_cast<const CoefCell *>(d);
  return 0;
}

// What tells the six calls apart.  A check leaves the locate fields null, an unrotated call the
// rotation at 0 and located_dev / dev_faults null, a call without the magics the magic fields null.
struct ScrubCall {
  const char *name;  // for messages
  bool rotated;
  int n_shift;
  long long first_stripe;
  bool locates;
  unsigned long long *hyp;
  unsigned char *located, *located_dev;
  unsigned *counts, *dev_faults;
  int flags;
  bool magics;            // lsec_check_magic_dev(_rotated): the MG kernels and their finalize launch
  uint8_t *magic;         // 4 bytes per stripe
  const uint8_t *expect;  // may be null
  uint8_t *bad;           // may be null
  unsigned *verdicts;     // may be null: [parity-bad, magic-bad]
};

template <typename Args>
constexpr bool kMagicScrub = std::is_same<Args, lsec::CheckMagicArgs>::value || std::is_same<Args, lsec::CheckMagicRotArgs>::value;

// the fields of an argument struct that change from launch to launch, for the one that starts at stripe s0
template <typename Args>
void scrub_launch_fields(Args &a, const ScrubCall &c, const lsec_shard_t *sh, unsigned *syndrome, long long s0, int nstripes,
                         uint32_t rot0) {
  const int n = a.K + a.R;
  a.nstripes = nstripes;
  a.syndrome = syndrome + s0;
  if constexpr (lsec::kLocArgs<Args>) a.hyp = c.hyp + s0;
  if constexpr (lsec::kRotArgs<Args>) {
    a.rot0 = rot0_from(rot0, a.rot_step, n, s0);
    for (int i = 0; i < n; ++i) a.sh[i] = shard_from(sh[i], s0);
  } else {
    for (int j = 0; j < a.K; ++j) a.in[j] = shard_from(sh[j], s0);
    for (int r = 0; r < a.R; ++r) a.par[r] = shard_from(sh[a.K + r], s0);
  }
}

// The accumulate launches: one per 32-bit range of tiles, in the encode's launch shape for K x R.
template <typename Args>
int enqueue_scrub(const ScrubCall &c, const lio_erasure_plan_t *p, const void *cells, const CoefCell *ratio, const lsec_shard_t *sh,
                  int nstripes, long long C, unsigned *syndrome, unsigned *bad_count, unsigned long long *acc, uint32_t rot0,
                  uint32_t rot_step, hipStream_t st) {
  Args a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.cells = static_cast<const CoefCell *>(cells);
  a.K = p->data_strips;
  a.R = p->parity_strips;
  a.size = C;
  a.packet = p->packet_size;
  a.bad_count = bad_count;
  if constexpr (lsec::kLocArgs<Args>) a.ratio = ratio;
  if constexpr (lsec::kRotArgs<Args>) {
    a.rot_step = rot_step;
    a.rot_n = static_cast<uint32_t>(a.K + a.R);
  }
  // the encode's dwords per lane for this shape (0: its packet network, which the check has no form of)
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  const int dw = sliced ? cauchy8_bitsliced_dw(a.K, a.R, C) : 0;
  return for_launches(nstripes, launch_stripes(C, c.rotated || c.magics), [&](long long s0, int ns) {
    scrub_launch_fields(a, c, sh, syndrome, s0, ns, rot0);
    hipError_t err;
    if constexpr (kMagicScrub<Args>) {
      a.magic_acc = acc + 2 * s0;
      err = sliced ? lsec::launch_check_magic_bitsliced(a, st, dw) : lsec::launch_check_magic_bytewise(a, st);
      if (err != hipSuccess) return fail("%s: kernel launch failed: %s", c.name, hipGetErrorString(err));
    } else {
      err = sliced ? lsec::launch_scrub_bitsliced(a, st, dw) : lsec::launch_scrub_bytewise(a, st);
      if (err != hipSuccess)
        return fail("%s%s kernel launch failed: %s", c.rotated ? "rotated " : "", c.locates ? "locate" : "check", hipGetErrorString(err));
    }
    return 0;
  });
}

// The tile launches and the finalize launch of a call with the magics, between the allocation and the
// release of its accumulators on the stream.
int enqueue_scrub_magic(const ScrubCall &c, const lio_erasure_plan_t *p, const void *cells, const lsec_shard_t *sh, int nstripes,
                        long long C, unsigned *syndrome, uint32_t rot0, uint32_t rot_step, hipStream_t st) {
  const int n = p->data_strips + p->parity_strips;
  unsigned long long *acc = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&acc), 16ull * nstripes, st);
  if (err == hipSuccess && (err = hipMemsetAsync(acc, 0, 16ull * nstripes, st)) != hipSuccess) (void)hipFreeAsync(acc, st);
  if (err != hipSuccess) return fail("%s: the magic accumulators (%llu bytes): %s", c.name, 16ull * nstripes, hipGetErrorString(err));
  int rc = 0;
  if (C > 0) {
    const auto enqueue = c.rotated ? enqueue_scrub<lsec::CheckMagicRotArgs> : enqueue_scrub<lsec::CheckMagicArgs>;
    rc = enqueue(c, p, cells, nullptr, sh, nstripes, C, syndrome, nullptr, acc, rot0, rot_step, st);
  }
  if (rc == 0) {
    err = lsec::launch_check_magic_finalize(acc, syndrome, nstripes, static_cast<int64_t>(n) * C, c.magic, c.expect, c.bad, c.verdicts, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", c.name, hipGetErrorString(err));
  }
  err = hipFreeAsync(acc, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the magic accumulators: %s", c.name, hipGetErrorString(err));
  return rc;
}

// Every limit's message names the limit; nothing is enqueued when one is passed.
int scrub_dev(PlanExt *e, const ScrubCall &c, const lsec_shard_t *sh, int nstripes, long long C, unsigned *syndrome,
              unsigned *bad_count, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", c.name,
                JE_method[p->method], p->w, kind);
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  if (k < 1 || k > lsec::kMaxK)
    return fail("%s: k=%d outside 1..%d (one launch's inputs%s)", c.name, k, lsec::kMaxK, c.locates ? ", one bit of hyp each" : "");
  if (c.locates && (m < 2 || m > 8))
    return fail("%s: m=%d outside 2..8 (one parity row cannot locate; one launch's parity rows)", c.name, m);
  if (m < 1 || m > 8) return fail("%s: m=%d outside 1..8 (one launch's parity rows)", c.name, m);
  if (c.flags & ~LSEC_LOCATE_REPAIR) return fail("%s: flags %#x has bits other than LSEC_LOCATE_REPAIR", c.name, c.flags);
  const bool repair = (c.flags & LSEC_LOCATE_REPAIR) != 0;
  // (the calls with the magics name themselves in every message; the older calls' messages stay as they are)
  const std::string pre_s = c.magics ? std::string(c.name) + ": " : std::string();
  const char *pre = pre_s.c_str();
  if (nstripes < 0) return fail("%snstripes %d is negative", pre, nstripes);
  if (c.n_shift < 0) return fail("%sn_shift %d is negative", pre, c.n_shift);
  if (c.first_stripe < 0) return fail("%sfirst_stripe %lld is negative", pre, c.first_stripe);
  if (check_geometry(p, C)) return c.magics ? named(c.name, -1) : -1;
  if (nstripes > 0 && !syndrome) return fail("%ssyndrome is NULL", pre);
  if (c.locates && nstripes > 0 && !c.hyp) return fail("hyp is NULL");
  if (c.locates && nstripes > 0 && !c.located) return fail("located is NULL");
  if (reinterpret_cast<uintptr_t>(syndrome) % 4 != 0)
    return fail("%ssyndrome %p is not a multiple of 4 bytes", pre, static_cast<void *>(syndrome));
  if (reinterpret_cast<uintptr_t>(bad_count) % 4 != 0) return fail("bad_count %p is not a multiple of 4 bytes", static_cast<void *>(bad_count));
  if (reinterpret_cast<uintptr_t>(c.hyp) % 8 != 0) return fail("hyp %p is not a multiple of 8 bytes", static_cast<void *>(c.hyp));
  if (reinterpret_cast<uintptr_t>(c.counts) % 4 != 0) return fail("counts %p is not a multiple of 4 bytes", static_cast<void *>(c.counts));
  if (reinterpret_cast<uintptr_t>(c.dev_faults) % 4 != 0) return fail("dev_faults %p is not a multiple of 4 bytes", static_cast<void *>(c.dev_faults));
  if (c.magics && nstripes > 0 && !c.magic) return fail("%s: magic is NULL (4 bytes per stripe, required with nstripes > 0)", c.name);
  if (reinterpret_cast<uintptr_t>(c.verdicts) % 4 != 0)
    return fail("%s: counts %p is not a multiple of 4 bytes (two 32-bit words)", c.name, static_cast<void *>(c.verdicts));
  const PatternTable *tab = nullptr;
  PatternTable::Dev dv;
  if (c.locates) {
    const lsec::gf8::Mat *q = nullptr;
    if (locate_ratio(e, &q)) return -1;  // a zero coefficient is refused here, before any device is touched
  }
  if (repair) {
    // The k+m single erasures of the logical chunks, in chunk order: located[s] is the stripe's pattern id,
    // both sentinels are past the table.  The limits above (k <= 64, m <= 8) are inside those of the
    // patterned decode, so the repair adds none.
    std::vector<int> singles;
    for (int i = 0; i < n; ++i) {
      singles.push_back(i);
      singles.push_back(-1);
    }
    if (nstripes == 0) {
      // preparing ahead: the matrix work always, the upload where there is a device to upload to
      int ndev = 0;
      if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        PatternTable host_only;
        return build_pattern_table(e, singles.data(), n, nullptr, 0, host_only);
      }
    }
    if (pattern_table_dev(e, singles.data(), n, nullptr, 0, &tab, &dv)) return -1;  // cached on the plan
  }
  if (nstripes == 0) return 0;
  const void *cells = nullptr;
  if (encode_image(e, &cells)) return -1;
  const int R = encode_rows(e);
  if (R != m) return fail("%s: the plan encodes %d parity rows, m=%d", c.name, R, m);
  const CoefCell *ratio = nullptr;
  if (c.locates && ratio_cells_dev(e, &ratio)) return -1;
  // the call sets every element itself, stripes of an empty chunk included (located and located_dev: the finalize launch)
  HIP_OK(hipMemsetAsync(syndrome, 0, sizeof(unsigned) * static_cast<size_t>(nstripes), st));
  if (bad_count) HIP_OK(hipMemsetAsync(bad_count, 0, sizeof(unsigned), st));
  if (c.locates) HIP_OK(hipMemsetAsync(c.hyp, 0xFF, sizeof(unsigned long long) * static_cast<size_t>(nstripes), st));
  if (c.counts) HIP_OK(hipMemsetAsync(c.counts, 0, 2 * sizeof(unsigned), st));
  if (c.dev_faults) HIP_OK(hipMemsetAsync(c.dev_faults, 0, sizeof(unsigned) * static_cast<size_t>(n), st));
  if (c.verdicts) HIP_OK(hipMemsetAsync(c.verdicts, 0, 2 * sizeof(unsigned), st));
  const uint32_t rot_step = c.rotated ? static_cast<uint32_t>(c.n_shift % n) : 0;
  const uint32_t rot0 = c.rotated ? pattern_rot0(n, c.n_shift, c.first_stripe) : 0;
  if (c.magics) return enqueue_scrub_magic(c, p, cells, sh, nstripes, C, syndrome, rot0, rot_step, st);
  if (C > 0) {
    const auto enqueue = c.rotated ? (c.locates ? enqueue_scrub<lsec::LocateRotArgs> : enqueue_scrub<lsec::CheckRotArgs>)
                                   : (c.locates ? enqueue_scrub<lsec::LocateArgs> : enqueue_scrub<lsec::CheckArgs>);
    if (enqueue(c, p, cells, ratio, sh, nstripes, C, syndrome, bad_count, nullptr, rot0, rot_step, st)) return -1;
  }
  if (!c.locates) return 0;
  const hipError_t err = c.rotated ? lsec::launch_locate_finalize_rot(syndrome, c.hyp, c.located, c.located_dev, c.counts, c.dev_faults,
                                                                      nstripes, k, R, rot0, rot_step, static_cast<uint32_t>(n), st)
                                   : lsec::launch_locate_finalize(syndrome, c.hyp, c.located, c.counts, nstripes, k, R, st);
  if (err != hipSuccess) return fail("%slocate finalize launch failed: %s", c.rotated ? "rotated " : "", hipGetErrorString(err));
  if (repair) return enqueue_patterns(e, *tab, dv, sh, nstripes, C, c.located, rot0, rot_step, c.rotated ? kRotSingles : kRotNone, st);
  return 0;
}

}  // namespace

int check_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, unsigned *syndrome, unsigned *bad_count,
              hipStream_t st) {
  const ScrubCall c = {"lsec_check_dev"};
  return scrub_dev(e, c, sh, nstripes, C, syndrome, bad_count, st);
}

int check_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                      unsigned *syndrome, unsigned *bad_count, hipStream_t st) {
  const ScrubCall c = {"lsec_check_dev_rotated", true, n_shift, first_stripe};
  return scrub_dev(e, c, devs, nstripes, C, syndrome, bad_count, st);
}

namespace {
// a check's ScrubCall with the magic fields filled in (mc.bad_count: the two verdict words)
ScrubCall with_magics(ScrubCall c, const MagicCheck &mc) {
  c.magics = true;
  c.magic = mc.magic;
  c.expect = mc.expect;
  c.bad = mc.bad;
  c.verdicts = mc.bad_count;
  return c;
}
}  // namespace

int check_magic_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, unsigned *syndrome, const MagicCheck &mc,
                    hipStream_t st) {
  const ScrubCall c = with_magics({"lsec_check_magic_dev"}, mc);
  return scrub_dev(e, c, sh, nstripes, C, syndrome, nullptr, st);
}

int check_magic_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                            unsigned *syndrome, const MagicCheck &mc, hipStream_t st) {
  const ScrubCall c = with_magics({"lsec_check_magic_dev_rotated", true, n_shift, first_stripe}, mc);
  return scrub_dev(e, c, devs, nstripes, C, syndrome, nullptr, st);
}

int locate_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, unsigned *syndrome, unsigned long long *hyp,
               unsigned char *located, unsigned *counts, int flags, hipStream_t st) {
  const ScrubCall c = {"lsec_locate_dev", false, 0, 0, true, hyp, located, nullptr, counts, nullptr, flags};
  return scrub_dev(e, c, sh, nstripes, C, syndrome, nullptr, st);
}

int locate_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                       unsigned *syndrome, unsigned long long *hyp, unsigned char *located, unsigned char *located_dev,
                       unsigned *counts, unsigned *dev_faults, int flags, hipStream_t st) {
  const ScrubCall c = {"lsec_locate_dev_rotated", true, n_shift, first_stripe, true, hyp, located, located_dev, counts, dev_faults, flags};
  return scrub_dev(e, c, devs, nstripes, C, syndrome, nullptr, st);
}

// ---------------------------------------------------------------- parity update, rotated or not
// lsec_update_dev: parity_r ^= sum_i g[r][cols[i]] * (old_i ^ fresh_i), and with LSEC_UPDATE_STORE
// old_i <- fresh_i, over the cached encode image: one launch per 32-bit range of tiles (as
// enqueue_scrub), nothing allocated or uploaded per call.  Only the c changed chunks, their fresh
// contents and the m parity chunks are looked at: every other entry of sh is never read, here or in
// the kernel.  One validation ladder, in the order of the header's refusal list; it touches no device.
//
// lsec_update_dev_rotated: the same over the k+m physical devices of a rotated LUN.  The kernels
// work each stripe's rotation out themselves (ec_kernels.h, UpdateRotArgs); every device holds a
// changed chunk or parity in some stripe, so all k+m entries are validated and travel.  Each later
// launch's rot0 advances by (s0 mod n) * rot_step, as the rotated check's.
//
// The two calls are one path (update_path) that an UpdateCall steers.
namespace {

// What tells the two calls apart.  The unrotated call leaves the rotation at 0.
struct UpdateCall {
  const char *name;  // for messages
  bool rotated;
  int n_shift;
  long long first_stripe;
  bool with_magic;  // the masked calls that keep the stripe magics (lsec_update_magic_dev_masked*)
  uint8_t *magic;   //   their 4 * nstripes bytes of device memory, in and out
};

// the launches: one per 32-bit range of tiles, in the update's own launch shape for R rows
template <typename Args>
int enqueue_update(const UpdateCall &uc, const lio_erasure_plan_t *p, const void *cells, const uint8_t *col, int c,
                   const lsec_shard_t *sh, const int *cols, const lsec_shard_t *fresh, int nstripes, long long C, int flags,
                   hipStream_t st) {
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  Args a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  std::memcpy(a.col, col, static_cast<size_t>(c));
  a.cells = static_cast<const CoefCell *>(cells);
  a.K = k;
  a.R = m;
  a.c = c;
  a.size = C;
  a.packet = p->packet_size;
  a.store = (flags & LSEC_UPDATE_STORE) ? 1 : 0;
  uint32_t rot0 = 0;
  if constexpr (lsec::kRotArgs<Args>) {
    a.rot_step = static_cast<uint32_t>(uc.n_shift % n);
    a.rot_n = static_cast<uint32_t>(n);
    rot0 = pattern_rot0(n, uc.n_shift, uc.first_stripe);
  }
  // the encode's dwords per lane for this shape (0: its packet network, which the update has no form of)
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  const int dw = sliced ? cauchy8_bitsliced_dw(k, m, C) : 0;
  return for_launches(nstripes, launch_stripes(C, true), [&](long long s0, int ns) {
    a.nstripes = ns;
    for (int i = 0; i < c; ++i) a.fresh[i] = shard_from(fresh[i], s0);
    hipError_t err;
    if constexpr (lsec::kRotArgs<Args>) {
      a.rot0 = rot0_from(rot0, a.rot_step, n, s0);
      for (int i = 0; i < n; ++i) a.sh[i] = shard_from(sh[i], s0);
      err = sliced ? lsec::launch_update_rot_bitsliced(a, st, dw) : lsec::launch_update_rot_bytewise(a, st);
    } else {
      for (int i = 0; i < c; ++i) a.old[i] = shard_from(sh[cols[i]], s0);
      for (int r = 0; r < m; ++r) a.par[r] = shard_from(sh[k + r], s0);
      err = sliced ? lsec::launch_update_bitsliced(a, st, dw) : lsec::launch_update_bytewise(a, st);
    }
    if (err != hipSuccess) return fail("%supdate kernel launch failed: %s", uc.rotated ? "rotated " : "", hipGetErrorString(err));
    return 0;
  });
}

int update_path(PlanExt *e, const UpdateCall &uc, const lsec_shard_t *sh, int nstripes, long long C, const int *cols,
                const lsec_shard_t *fresh, int flags, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", uc.name,
                JE_method[p->method], p->w, kind);
  const int k = p->data_strips, m = p->parity_strips;
  if (k < 1 || k > lsec::kMaxK) return fail("%s: k=%d outside 1..%d (one launch's columns)", uc.name, k, lsec::kMaxK);
  if (m < 1 || m > 8) return fail("%s: m=%d outside 1..8 (one launch's parity rows)", uc.name, m);
  if (!sh) return fail("%s is NULL", uc.rotated ? "devs" : "shards");
  if (!cols) return fail("cols is NULL");
  if (!fresh) return fail("fresh is NULL");
  if (cols[0] == -1) return fail("%s: cols is empty (1..k=%d changed data chunks)", uc.name, k);
  uint8_t col[lsec::kMaxK];
  unsigned long long seen = 0;
  int c = 0;
  for (; cols[c] != -1; ++c) {
    if (c == k) return fail("%s: cols lists more than k=%d chunks", uc.name, k);
    const int id = cols[c];
    if (id < 0) return fail("%s: cols[%d] = %d is negative (data chunk ids are 0..%d)", uc.name, c, id, k - 1);
    if (id >= k)
      return fail("%s: cols[%d] = %d is not a data chunk (ids are 0..%d; %d..%d are parity)", uc.name, c, id, k - 1, k, k + m - 1);
    if (seen >> id & 1) return fail("%s: cols lists chunk %d twice (ids must be distinct)", uc.name, id);
    seen |= 1ull << id;
    col[c] = static_cast<uint8_t>(id);
  }
  if (flags & ~LSEC_UPDATE_STORE) return fail("%s: flags %#x has bits other than LSEC_UPDATE_STORE", uc.name, flags);
  if (uc.n_shift < 0) return fail("n_shift %d is negative", uc.n_shift);
  if (uc.first_stripe < 0) return fail("first_stripe %lld is negative", uc.first_stripe);
  const auto aligned = [&](const char *what, int i, const lsec_shard_t &s) {
    if (reinterpret_cast<uintptr_t>(s.base) % 8 != 0)
      return fail("%s %d: base %p is not a multiple of 8 bytes (lsec_shard_t)", what, i, s.base);
    if (nstripes > 1 && s.stride % 8 != 0)
      return fail("%s %d: stride %lld is not a multiple of 8 bytes (lsec_shard_t)", what, i, s.stride);
    return 0;
  };
  if (uc.rotated) {
    // every device holds a changed chunk in some stripe and parity in others: all k+m are used
    for (int i = 0; i < k + m; ++i)
      if (aligned("device", i, sh[i])) return -1;
    for (int i = 0; i < c; ++i)
      if (aligned("fresh", i, fresh[i])) return -1;
  } else {
    for (int i = 0; i < c; ++i)
      if (aligned("shard", cols[i], sh[cols[i]]) || aligned("fresh", i, fresh[i])) return -1;
    for (int r = 0; r < m; ++r)
      if (aligned("shard", k + r, sh[k + r])) return -1;
  }
  if (check_geometry(p, C)) return -1;
  if (nstripes < 0) return fail("nstripes %d is negative", nstripes);
  if (nstripes == 0) return 0;
  const void *cells = nullptr;
  if (encode_image(e, &cells)) return -1;
  const int R = encode_rows(e);
  if (R != m) return fail("%s: the plan encodes %d parity rows, m=%d", uc.name, R, m);
  if (C == 0) return 0;
  const auto enqueue = uc.rotated ? enqueue_update<lsec::UpdateRotArgs> : enqueue_update<lsec::UpdateArgs>;
  return enqueue(uc, p, cells, col, c, sh, cols, fresh, nstripes, C, flags, st);
}

}  // namespace

int update_dev(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, const int *cols, const lsec_shard_t *fresh,
               int flags, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_dev"};
  return update_path(e, uc, sh, nstripes, C, cols, fresh, flags, st);
}

int update_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                       const int *cols, const lsec_shard_t *fresh, int flags, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_dev_rotated", true, n_shift, first_stripe};
  return update_path(e, uc, devs, nstripes, C, cols, fresh, flags, st);
}

// ---------------------------------------------------------------- parity update, a changed set per stripe
// lsec_update_dev_masked / lsec_update_dev_masked_rotated: the update with one 64-bit word per stripe
// (bit j: data chunk j changes) in device memory, and fresh indexed by logical chunk id.  A column is
// enabled when it has a fresh buffer; the kernels AND every stripe's word with the enabled columns
// below k (ec_kernels.h, UpdateMaskArgs), so only enabled columns travel and are validated.  One path
// for both calls, steered by an UpdateCall; the unrotated call runs the same kernels with every
// rotation 0.  One validation ladder, in the order of the header's refusal list; it touches no
// device.  Launches as enqueue_update's: per launch the mask pointer advances by s0 words and rot0
// by (s0 mod n) * rot_step.  Nothing is allocated or uploaded per call.
//
// lsec_update_magic_dev_masked / _rotated are the same path with UpdateCall::with_magic: the MG kernels
// (ec_kernels.h, UpdateMaskMagicArgs) in place of the plain ones, over 16 bytes per stripe of
// accumulators from the stream-ordered allocator -- zeroed before the first launch, advancing by
// 2 * s0 words per launch, freed on the stream -- and one finalize launch behind the tile launches
// that takes the mask pointer and the enabled columns of the whole call.
namespace {

int update_masked_path(PlanExt *e, const UpdateCall &uc, const lsec_shard_t *sh, int nstripes, long long C,
                       const unsigned long long *stripe_cols, const lsec_shard_t *fresh, int flags, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", uc.name,
                JE_method[p->method], p->w, kind);
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  if (k < 1 || k > lsec::kMaxK) return fail("%s: k=%d outside 1..%d (one mask word's columns)", uc.name, k, lsec::kMaxK);
  if (m < 1 || m > 8) return fail("%s: m=%d outside 1..8 (one launch's parity rows)", uc.name, m);
  if (!sh) return fail("%s: %s is NULL", uc.name, uc.rotated ? "devs" : "shards");
  if (!fresh) return fail("%s: fresh is NULL", uc.name);
  if (flags & ~LSEC_UPDATE_STORE) return fail("%s: flags %#x has bits other than LSEC_UPDATE_STORE", uc.name, flags);
  if (uc.n_shift < 0) return fail("%s: n_shift %d is negative", uc.name, uc.n_shift);
  if (uc.first_stripe < 0) return fail("%s: first_stripe %lld is negative", uc.name, uc.first_stripe);
  // the enabled columns below k, in one word (k = 64: every bit, and no shift by 64)
  unsigned long long allowed = 0;
  for (int j = 0; j < k; ++j)
    if (fresh[j].base) allowed |= 1ull << j;
  if (nstripes > 0 && !allowed)
    return fail("%s: no enabled column (fresh[j].base is NULL for every j < k=%d)", uc.name, k);
  const auto aligned = [&](const char *what, int i, const lsec_shard_t &s) {
    if (reinterpret_cast<uintptr_t>(s.base) % 8 != 0)
      return fail("%s: %s %d: base %p is not a multiple of 8 bytes (lsec_shard_t)", uc.name, what, i, s.base);
    if (nstripes > 1 && s.stride % 8 != 0)
      return fail("%s: %s %d: stride %lld is not a multiple of 8 bytes (lsec_shard_t)", uc.name, what, i, s.stride);
    return 0;
  };
  for (int j = 0; j < k; ++j)
    if ((allowed >> j & 1) && aligned("fresh", j, fresh[j])) return -1;
  if (uc.rotated) {
    // every device holds a changed chunk in some stripe and parity in others: all k+m are used
    for (int i = 0; i < n; ++i)
      if (aligned("device", i, sh[i])) return -1;
  } else {
    for (int j = 0; j < k; ++j) {
      if (!(allowed >> j & 1)) continue;  // a column that is not enabled: its entry is ignored entirely
      if (nstripes > 0 && !sh[j].base) return fail("%s: shard %d: base is NULL, and fresh[%d] is given", uc.name, j, j);
      if (aligned("shard", j, sh[j])) return -1;
    }
    for (int r = 0; r < m; ++r)
      if (aligned("shard", k + r, sh[k + r])) return -1;
  }
  if (nstripes > 0 && !stripe_cols) return fail("%s: stripe_cols is NULL", uc.name);
  if (nstripes > 0 && reinterpret_cast<uintptr_t>(stripe_cols) % 8 != 0)
    return fail("%s: stripe_cols %p is not a multiple of 8 bytes (64-bit words)", uc.name, static_cast<const void *>(stripe_cols));
  if (uc.with_magic && nstripes > 0 && !uc.magic) return fail("%s: magic is NULL", uc.name);
  if (check_geometry(p, C)) {
    const std::string why = tl_err;  // the shared rule's message, behind the call's name
    return fail("%s: %s", uc.name, why.c_str());
  }
  if (nstripes < 0) return fail("%s: nstripes %d is negative", uc.name, nstripes);
  if (nstripes == 0) return 0;
  const void *cells = nullptr;
  if (encode_image(e, &cells)) return -1;
  const int R = encode_rows(e);
  if (R != m) return fail("%s: the plan encodes %d parity rows, m=%d", uc.name, R, m);
  if (C == 0) return 0;
  lsec::UpdateMaskMagicArgs a;  // (the plain call's launches take its UpdateMaskArgs part)
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.cells = static_cast<const CoefCell *>(cells);
  a.K = k;
  a.R = m;
  a.size = C;
  a.packet = p->packet_size;
  a.store = (flags & LSEC_UPDATE_STORE) ? 1 : 0;
  a.allowed = allowed;
  a.rot_step = uc.rotated ? static_cast<uint32_t>(uc.n_shift % n) : 0;
  a.rot_n = static_cast<uint32_t>(n);
  const uint32_t rot0 = uc.rotated ? pattern_rot0(n, uc.n_shift, uc.first_stripe) : 0;
  // the encode's dwords per lane for this shape (0: its packet network, which the update has no form of)
  const bool sliced = kind == KBITSLICED;
  const int dw = sliced ? cauchy8_bitsliced_dw(k, m, C) : 0;
  unsigned long long *acc = nullptr;  // with_magic: each stripe's change of the two halves
  if (uc.with_magic) {
    hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&acc), 16ull * nstripes, st);
    if (err == hipSuccess && (err = hipMemsetAsync(acc, 0, 16ull * nstripes, st)) != hipSuccess) (void)hipFreeAsync(acc, st);
    if (err != hipSuccess) return fail("%s: the magic accumulators (%llu bytes): %s", uc.name, 16ull * nstripes, hipGetErrorString(err));
  }
  int rc = for_launches(nstripes, launch_stripes(C, true), [&](long long s0, int ns) {
    a.nstripes = ns;
    a.stripe_cols = stripe_cols + s0;
    a.magic_acc = acc ? acc + 2 * s0 : nullptr;
    a.rot0 = rot0_from(rot0, a.rot_step, n, s0);
    for (int j = 0; j < k; ++j)
      if (allowed >> j & 1) a.fresh[j] = shard_from(fresh[j], s0);
    // (unrotated: the refs of the columns that are not enabled stay zero, and no kernel addresses them)
    for (int i = 0; i < n; ++i)
      if (uc.rotated || i >= k || (allowed >> i & 1)) a.sh[i] = shard_from(sh[i], s0);
    const hipError_t err = uc.with_magic ? (sliced ? lsec::launch_update_magic_bitsliced(a, st, dw) : lsec::launch_update_magic_bytewise(a, st))
                                         : (sliced ? lsec::launch_update_masked_bitsliced(a, st, dw) : lsec::launch_update_masked_bytewise(a, st));
    if (err != hipSuccess) return fail("%s: kernel launch failed: %s", uc.name, hipGetErrorString(err));
    return 0;
  });
  if (!uc.with_magic) return rc;
  if (rc == 0) {
    const hipError_t err = lsec::launch_update_magic_finalize(acc, stripe_cols, allowed, nstripes, uc.magic, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", uc.name, hipGetErrorString(err));
  }
  const hipError_t err = hipFreeAsync(acc, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the magic accumulators: %s", uc.name, hipGetErrorString(err));
  return rc;
}

}  // namespace

int update_dev_masked(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, const unsigned long long *stripe_cols,
                      const lsec_shard_t *fresh, int flags, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_dev_masked"};
  return update_masked_path(e, uc, sh, nstripes, C, stripe_cols, fresh, flags, st);
}

int update_dev_masked_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift,
                              long long first_stripe, const unsigned long long *stripe_cols, const lsec_shard_t *fresh,
                              int flags, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_dev_masked_rotated", true, n_shift, first_stripe};
  return update_masked_path(e, uc, devs, nstripes, C, stripe_cols, fresh, flags, st);
}

int update_magic_dev_masked(PlanExt *e, const lsec_shard_t *sh, int nstripes, long long C, const unsigned long long *stripe_cols,
                            const lsec_shard_t *fresh, int flags, uint8_t *magic, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_magic_dev_masked", false, 0, 0, true, magic};
  return update_masked_path(e, uc, sh, nstripes, C, stripe_cols, fresh, flags, st);
}

int update_magic_dev_masked_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift,
                                    long long first_stripe, const unsigned long long *stripe_cols, const lsec_shard_t *fresh,
                                    int flags, uint8_t *magic, hipStream_t st) {
  const UpdateCall uc = {"lsec_update_magic_dev_masked_rotated", true, n_shift, first_stripe, true, magic};
  return update_masked_path(e, uc, devs, nstripes, C, stripe_cols, fresh, flags, st);
}

// ---------------------------------------------------------------- encode over a rotated LUN
// lsec_encode_dev_rotated: the parity rows lsec_encode_dev writes for the logical view of every
// stripe, written to the devices that hold them (ec_kernels.h, EncodeRotArgs).  Validated as the
// rotated check, minus its outputs; the launches are the rotated check's too (one per 32-bit range
// of tiles, rot0 advancing from launch to launch), over the cached encode image.  A Cauchy plan
// takes the bit-sliced table kernel at every shape, as the check does: the compiled packet
// networks have no rotated form, and the bytes are the same.
//
// lsec_encode_magic_dev_rotated: the same pass with the MG kernels (ec_kernels.h, EncodeMagicRotArgs),
// which also sum each stripe's adler32 magic from the chunks the encode holds in registers, over 16
// bytes per stripe of accumulators from the stream-ordered allocator -- zeroed before the first launch,
// advancing by 2 * s0 words per launch, freed on the stream -- and launch_magic_finalize behind the tile
// launches.  Its one rung of its own, a NULL magic, sits behind the plain call's, and every message of
// its carries the call's name.
//
// The two calls are one path (encode_rot_path) that an EncodeRotCall steers.
namespace {

struct EncodeRotCall {
  const char *name;  // for messages
  bool magics;       // lsec_encode_magic_dev_rotated: the MG kernels and the finalize launch
  uint8_t *magic;    // 4 bytes per stripe
};

// The tile launches: one per 32-bit range of tiles, in the rotated check's launch shape for K x R.
// acc: the magic accumulators of the whole call (Args = EncodeMagicRotArgs), else unused.
template <typename Args>
int enqueue_encode_rot(const EncodeRotCall &c, const lio_erasure_plan_t *p, const void *cells, const lsec_shard_t *devs, int nstripes,
                       long long C, int n_shift, long long first_stripe, unsigned long long *acc, hipStream_t st) {
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  Args a;
  std::memset(static_cast<void *>(&a), 0, sizeof(a));
  a.cells = static_cast<const CoefCell *>(cells);
  a.K = k;
  a.R = m;
  a.size = C;
  a.packet = p->packet_size;
  a.rot_step = static_cast<uint32_t>(n_shift % n);
  a.rot_n = static_cast<uint32_t>(n);
  const uint32_t rot0 = pattern_rot0(n, n_shift, first_stripe);
  // the encode's dwords per lane for this shape (0: its packet network, which the rotated encode has no form of)
  const bool sliced = kernel_kind(p->method, p->w) == KBITSLICED;
  const int dw = sliced ? cauchy8_bitsliced_dw(k, m, C) : 0;
  return for_launches(nstripes, launch_stripes(C, true), [&](long long s0, int ns) {
    a.nstripes = ns;
    a.rot0 = rot0_from(rot0, a.rot_step, n, s0);
    for (int i = 0; i < n; ++i) a.sh[i] = shard_from(devs[i], s0);
    if constexpr (std::is_same<Args, lsec::EncodeMagicRotArgs>::value) {
      a.magic_acc = acc + 2 * s0;
      const hipError_t err = sliced ? lsec::launch_encode_magic_rot_bitsliced(a, st, dw) : lsec::launch_encode_magic_rot_bytewise(a, st);
      if (err != hipSuccess) return fail("%s: kernel launch failed: %s", c.name, hipGetErrorString(err));
    } else {
      const hipError_t err = sliced ? lsec::launch_encode_rot_bitsliced(a, st, dw) : lsec::launch_encode_rot_bytewise(a, st);
      if (err != hipSuccess) return fail("rotated encode kernel launch failed: %s", hipGetErrorString(err));
    }
    return 0;
  });
}

// Every limit's message names the limit; nothing is enqueued when one is passed.
int encode_rot_path(PlanExt *e, const EncodeRotCall &c, const lsec_shard_t *devs, int nstripes, long long C, int n_shift,
                    long long first_stripe, hipStream_t st) {
  lsec::launch_record_reset();  // (lsec_test_launch_record)
  lio_erasure_plan_t *p = &e->pub;
  const int kind = kernel_kind(p->method, p->w);
  if (kind != KBYTEWISE && kind != KBITSLICED)
    return fail("%s needs plan kernel 1 (bytewise GF(2^8)) or 2 (bit-sliced GF(2^8)); %s (w=%d) is plan kernel %d", c.name,
                JE_method[p->method], p->w, kind);
  const int k = p->data_strips, m = p->parity_strips, n = k + m;
  if (k < 1 || k > lsec::kMaxK) return fail("%s: k=%d outside 1..%d (one launch's inputs)", c.name, k, lsec::kMaxK);
  if (m < 1 || m > 8) return fail("%s: m=%d outside 1..8 (one launch's parity rows)", c.name, m);
  // (the call with the magics names itself in every message; the plain call's messages stay as they are)
  const std::string pre_s = c.magics ? std::string(c.name) + ": " : std::string();
  const char *pre = pre_s.c_str();
  if (nstripes < 0) return fail("%snstripes %d is negative", pre, nstripes);
  if (n_shift < 0) return fail("%sn_shift %d is negative", pre, n_shift);
  if (first_stripe < 0) return fail("%sfirst_stripe %lld is negative", pre, first_stripe);
  if (check_geometry(p, C)) return c.magics ? named(c.name, -1) : -1;
  if (c.magics && nstripes > 0 && !c.magic) return fail("%s: magic is NULL (4 bytes per stripe, required with nstripes > 0)", c.name);
  if (nstripes == 0) return 0;
  const void *cells = nullptr;
  if (encode_image(e, &cells)) return -1;
  const int R = encode_rows(e);
  if (R != m) return fail("%s: the plan encodes %d parity rows, m=%d", c.name, R, m);
  if (!c.magics) return C == 0 ? 0 : enqueue_encode_rot<lsec::EncodeRotArgs>(c, p, cells, devs, nstripes, C, n_shift, first_stripe, nullptr, st);
  // the tile launches and the finalize launch, between the allocation and the release of the accumulators on the
  // stream; an empty chunk launches the finalize alone, over zero sums: every word 1, adler32 of nothing
  unsigned long long *acc = nullptr;
  hipError_t err = hipMallocAsync(reinterpret_cast<void **>(&acc), 16ull * nstripes, st);
  if (err == hipSuccess && (err = hipMemsetAsync(acc, 0, 16ull * nstripes, st)) != hipSuccess) (void)hipFreeAsync(acc, st);
  if (err != hipSuccess) return fail("%s: the magic accumulators (%llu bytes): %s", c.name, 16ull * nstripes, hipGetErrorString(err));
  int rc = C > 0 ? enqueue_encode_rot<lsec::EncodeMagicRotArgs>(c, p, cells, devs, nstripes, C, n_shift, first_stripe, acc, st) : 0;
  if (rc == 0) {
    err = lsec::launch_magic_finalize(acc, nstripes, static_cast<int64_t>(n) * C, c.magic, st);
    if (err != hipSuccess) rc = fail("%s: finalize launch failed: %s", c.name, hipGetErrorString(err));
  }
  err = hipFreeAsync(acc, st);
  if (err != hipSuccess && rc == 0) rc = fail("%s: freeing the magic accumulators: %s", c.name, hipGetErrorString(err));
  return rc;
}

}  // namespace

int encode_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                       hipStream_t st) {
  const EncodeRotCall c = {"lsec_encode_dev_rotated", false, nullptr};
  return encode_rot_path(e, c, devs, nstripes, C, n_shift, first_stripe, st);
}

int encode_magic_dev_rotated(PlanExt *e, const lsec_shard_t *devs, int nstripes, long long C, int n_shift, long long first_stripe,
                             uint8_t *magic, hipStream_t st) {
  const EncodeRotCall c = {"lsec_encode_magic_dev_rotated", true, magic};
  return encode_rot_path(e, c, devs, nstripes, C, n_shift, first_stripe, st);
}

}  // namespace eng

using namespace eng;

int set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  tl_err = buf;
  return -1;
}


void make_word_cell(uint32_t c, int w, uint32_t *out) {
  for (int b = 0; b < w; ++b, c = gfw::times_x(c, w)) out[b] = (w == 16) ? (c | (c << 16)) : c;
}

void make_cell(uint8_t c, CoefCell &cell) {
  uint8_t ta[8], tb[8], tc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int n = 0; n < 8; ++n) {
    ta[n] = gf8::mul(c, static_cast<uint8_t>(n));
    tb[n] = gf8::mul(c, static_cast<uint8_t>(n << 3));
    if (n < 4) tc[n] = gf8::mul(c, static_cast<uint8_t>(n << 6));
  }
  auto pack = [](const uint8_t *b) {
    return static_cast<uint32_t>(b[0]) | (static_cast<uint32_t>(b[1]) << 8) | (static_cast<uint32_t>(b[2]) << 16) |
           (static_cast<uint32_t>(b[3]) << 24);
  };
  cell.coef = c;
  cell.pad = 0;
  cell.ta_lo = pack(ta);
  cell.ta_hi = pack(ta + 4);
  cell.tb_lo = pack(tb);
  cell.tb_hi = pack(tb + 4);
  cell.tc_lo = pack(tc);
  cell.tc_hi = pack(tc + 4);
}
}  // namespace lsec

using namespace lsec::eng;

extern "C" {

int nearest_prime(int w, int which) {
  static const int primes[55] = {2,   3,   5,   7,   11,  13,  17,  19,  23,  29,  31,  37,  41,  43,
                                 47,  53,  59,  61,  67,  71,  73,  79,  83,  89,  97,  101, 103, 107,
                                 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181,
                                 191, 193, 197, 199, 211, 223, 227, 229, 233, 239, 241, 251, 257};
  // first prime >= w among primes[1..54]; which>0 -> it, which<0 -> the one below,
  // which==0 -> the closer of the two (ties go up)  (erasure_tools.c:50-77)
  for (int i = 1; i < 55; ++i) {
    if (w > primes[i]) continue;
    if (which > 0) return primes[i];
    if (which < 0) return primes[i - 1];
    return (w - primes[i - 1] < primes[i] - w) ? primes[i - 1] : primes[i];
  }
  return primes[54];
}

int et_method_type(char *meth) {
  if (!meth) return -1;
  for (int i = 0; i < N_JE_METHODS; ++i)
    if (strcasecmp(meth, JE_method[i]) == 0) return i;
  return -1;
}

lio_erasure_plan_t *et_new_plan(int method, long long int strip_size, int data_strips, int parity_strips, int w,
                                int packet_size, int base_unit) {
  if (method < 0 || method >= N_JE_METHODS) {
    fail("et_new_plan: invalid method %d", method);
    return nullptr;
  }
  PlanExt *e = static_cast<PlanExt *>(calloc(1, sizeof(PlanExt)));
  if (!e) return nullptr;
  e->magic = kPlanMagic;
  e->impl = new PlanImpl();
  lio_erasure_plan_t *p = &e->pub;
  p->method = method;
  p->strip_size = strip_size;
  p->data_strips = data_strips;
  p->parity_strips = parity_strips;
  p->w = w;
  p->base_unit = base_unit;
  p->packet_size = packet_size;
  if (method == RAID4) {
    p->form_encoding_matrix = fp_dummy;
    p->form_decoding_matrix = fp_dummy;
  } else {
    p->form_encoding_matrix = fp_form_encoding;
    p->form_decoding_matrix = fp_form_decoding;
  }
  p->encode_block = fp_encode_block;
  p->decode_block = fp_decode_block;
  return p;
}

void et_destroy_plan(lio_erasure_plan_t *p) {
  if (!p) return;
  PlanExt *e = ext_of(p);
  free(p->encode_matrix);
  free(p->encode_bitmatrix);
  if (p->encode_schedule) {
    int i = 0;
    for (; p->encode_schedule[i][0] != -1; ++i) free(p->encode_schedule[i]);
    free(p->encode_schedule[i]);
    free(p->encode_schedule);
  }
  if (e) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    e->impl->for_each_image([](DevImage &img) { img.release(); });
    if (cur >= 0) (void)hipSetDevice(cur);
    delete e->impl;
    e->magic = 0;
  }
  free(e ? static_cast<void *>(e) : static_cast<void *>(p));
}

lio_erasure_plan_t *et_generate_plan(long long int file_size, int method, int data_strips, int parity_strips, int w,
                                     int packet_low, int packet_high) {
  int base_unit = 8;
  if (w == -1) {  // auto word size (erasure_tools.c:746-776)
    switch (method) {
      case REED_SOL_R6_OP: case REED_SOL_VAN: case CAUCHY_ORIG: case CAUCHY_GOOD: case LIBER8TION:
        w = 8;
        break;
      case BLAUM_ROTH: w = nearest_prime(data_strips + 1, 1) - 1; break;
      case LIBERATION: w = nearest_prime(data_strips, 1); break;
      case RAID4: w = 8; base_unit = 1; break;
      default:
        fail("et_generate_plan: invalid method %d", method);
        return nullptr;
    }
  }
  // search range (erasure_tools.c:779-796)
  const long long approx = file_size / (static_cast<long long>(w) * base_unit * data_strips);
  const int plow = approx < 4 * 1024 ? static_cast<int>(approx / 4) : 512;
  const int phigh = approx < 4 * 1024 ? static_cast<int>(approx) : 4096;
  if (packet_low < 0) packet_low = plow;
  if (packet_high < 0) packet_high = phigh;
  if (packet_low > packet_high) {
    fail("et_generate_plan: packet_low > packet_high (%d > %d)", packet_low, packet_high);
    return nullptr;
  }
  packet_low = (packet_low / base_unit) * base_unit;
  packet_high = (packet_high / base_unit) * base_unit;
  // validation (erasure_tools.c:801-872)
  switch (method) {
    case REED_SOL_R6_OP:
      if (parity_strips != 2) { fail("%s needs parity_strips == 2", JE_method[method]); return nullptr; }
      [[fallthrough]];
    case REED_SOL_VAN: case CAUCHY_ORIG: case CAUCHY_GOOD:
      if (w != 8 && w != 16 && w != 32) { fail("%s needs w in {8,16,32}", JE_method[method]); return nullptr; }
      break;
    case BLAUM_ROTH:
      if (data_strips > w || nearest_prime(w + 1, 0) != w + 1 || packet_high % 8 != 0) {
        fail("blaum_roth: need k <= w, w+1 prime, packet %% 8 == 0");
        return nullptr;
      }
      break;
    case LIBERATION:
      if (data_strips > w || nearest_prime(w, 0) != w || packet_high % 8 != 0) {
        fail("liberation: need k <= w, w prime, packet %% 8 == 0");
        return nullptr;
      }
      break;
    case LIBER8TION:
      if (w != 8 || parity_strips != 2 || data_strips > w) { fail("liber8tion: need w == 8, m == 2, k <= 8"); return nullptr; }
      break;
    case RAID4:
      if (parity_strips != 1) { fail("raid4 needs parity_strips == 1"); return nullptr; }
      base_unit = 1;
      packet_low = 0;
      packet_high = 1;
      break;
    default:
      fail("et_generate_plan: invalid method %d", method);
      return nullptr;
  }
  // packet search: least padding, ties to the smaller packet, stop below 1 % (erasure_tools.c:876-896)
  long long best_excess = 10 * file_size, best_size = 0;
  int best_packet = -1;
  for (int ps = packet_high; ps > packet_low; ps -= base_unit) {
    const long long unit = static_cast<long long>(data_strips) * w * ps * base_unit;
    long long size = file_size;
    const long long rem = size % unit;
    if (rem > 0) size += unit - rem;
    const int excess = static_cast<int>(size - file_size);
    if (excess <= best_excess) {
      best_excess = excess;
      best_packet = ps;
      best_size = size;
      // `float increase = (1.0*j) / file_size * 100`: double arithmetic, then stored to a
      // float, which is what the < 1 test sees (erasure_tools.c:741, :893-894)
      const float increase = static_cast<float>((1.0 * excess) / file_size * 100);
      if (increase < 1) break;
    }
  }
  // Refused at plan time instead of failing on every block later (the segment maps a NULL plan
  // to -7 at exnode load, segment/jerasure.c:2237-2240):
  //  * packet codes asked for k equal chunks (file_size = k*C, what the segment passes,
  //    :2236) whose C is not a multiple of w * packet_size: the reference builds them, and its
  //    schedule encode then runs past the chunks (jerasure.c:1193-1207 walks strip_size > C
  //    bytes).  A file_size that is not k equal chunks is a file-tool request (et_encode pads
  //    the last strip to strip_size, erasure_tools.c:339-436) and keeps its padded plan.
  //  * plans no GPU kernel serves (there is no CPU path)
  const int kind = kernel_kind(method, w);
  if (kind == KNONE) {
    fail("et_generate_plan: %s at w=%d has no GPU kernel in this build", JE_method[method], w);
    return nullptr;
  }
  if (data_strips < 1 || parity_strips < 1 || data_strips + parity_strips > max_devs(method, w)) {
    fail("et_generate_plan: k=%d m=%d: k+m outside the engine's 2..%d at w=%d", data_strips, parity_strips,
         max_devs(method, w), w);
    return nullptr;
  }
  if (packet_kind(kind) && best_size != file_size && file_size % data_strips == 0) {
    fail("et_generate_plan: %s chunk %lld is not a multiple of w*packet_size = %d (the search padded %lld to %lld)",
         JE_method[method], file_size / data_strips, w * best_packet, file_size, best_size);
    return nullptr;
  }
  return et_new_plan(method, best_size / data_strips, data_strips, parity_strips, w, best_packet, base_unit);
}

// ---- file tools (erasure_tools.c:339-600): same file layout and padding ('0' bytes past EOF)
static size_t bread(char *buf, size_t n, FILE *f) {
  const size_t got = fread(buf, 1, n, f);
  if (got < n) memset(buf + got, '0', n - got);  // BLANK_CHAR, erasure_tools.c:37
  return n;
}

static int file_block(const lio_erasure_plan_t *p, int buffer_size) {
  const int unit = (p->data_strips + p->parity_strips) * p->w * p->packet_size * p->base_unit;
  if (unit <= 0) return -1;
  if (buffer_size == 0) buffer_size = 10 * 1024 * 1024;
  int j = buffer_size / unit;
  if (j == 0) j = 1;
  return j * unit / (p->data_strips + p->parity_strips);
}

int et_encode(lio_erasure_plan_t *plan, const char *fname, long long int foffset, const char *pname,
              long long int poffset, int buffer_size) {
  if (!ext_of(plan)) return fail("not an lstore_ec plan"), 1;
  FILE *fd = fopen(fname, "r");
  if (!fd) return fail("et_encode: cannot open %s", fname), 1;
  FILE *fp = fopen(pname, "r+");
  if (!fp) fp = fopen(pname, "w");
  if (!fp) { fclose(fd); return fail("et_encode: cannot open %s", pname), 1; }
  plan->form_encoding_matrix(plan);
  const int k = plan->data_strips, m = plan->parity_strips;
  const int block = file_block(plan, buffer_size);
  std::vector<char> buf(static_cast<size_t>(block) * (k + m));
  std::vector<char *> ptr(k + m);
  for (int i = 0; i < k + m; ++i) ptr[i] = buf.data() + static_cast<size_t>(i) * block;
  int rc = 0;
  for (long long rpos = 0, apos = foffset, ppos = poffset; rpos < plan->strip_size && rc == 0;
       rpos += block, apos += block, ppos += block) {
    const int bsize = static_cast<int>(std::min<long long>(block, plan->strip_size - rpos));
    for (int i = 0; i < k; ++i) {
      fseek(fd, apos + i * plan->strip_size, SEEK_SET);
      bread(ptr[i], bsize, fd);
    }
    if (encode_stripes_impl(ext_of(plan), ptr.data(), 1, bsize)) { rc = 1; break; }
    for (int i = 0; i < m; ++i) {
      fseek(fp, ppos + i * plan->strip_size, SEEK_SET);
      if (fwrite(ptr[k + i], 1, bsize, fp) != static_cast<size_t>(bsize)) rc = 1;
    }
  }
  fclose(fd);
  fclose(fp);
  return rc;
}

int et_decode(lio_erasure_plan_t *plan, long long int fsize, const char *fname, long long int foffset,
              const char *pname, long long int poffset, int buffer_size, int *erasures) {
  if (!ext_of(plan)) return fail("not an lstore_ec plan"), 1;
  const int k = plan->data_strips, m = plan->parity_strips;
  std::vector<int> missing(k + m, 0);
  int n = 0;
  for (; erasures[n] != -1; ++n) {
    if (erasures[n] < 0 || erasures[n] >= k + m) return fail("erasure id out of range"), 1;
    missing[erasures[n]] = 1;
  }
  if (n == 0) return 0;
  FILE *fd = fopen(fname, "r+");
  if (!fd) return fail("et_decode: cannot open %s", fname), 1;
  FILE *fp = fopen(pname, "r+");
  if (!fp) { fclose(fd); return fail("et_decode: cannot open %s", pname), 1; }
  plan->form_decoding_matrix(plan);
  const int block = file_block(plan, buffer_size);
  std::vector<char> buf(static_cast<size_t>(block) * (k + m));
  std::vector<char *> ptr(k + m);
  for (int i = 0; i < k + m; ++i) ptr[i] = buf.data() + static_cast<size_t>(i) * block;
  int rc = 0;
  for (long long rpos = 0, apos = foffset, ppos = poffset; rpos < plan->strip_size && rc == 0;
       rpos += block, apos += block, ppos += block) {
    const int bsize = static_cast<int>(std::min<long long>(block, plan->strip_size - rpos));
    for (int i = 0; i < k; ++i)
      if (!missing[i]) {
        fseek(fd, apos + i * plan->strip_size, SEEK_SET);
        bread(ptr[i], bsize, fd);
      }
    for (int i = 0; i < m; ++i)
      if (!missing[k + i]) {
        fseek(fp, ppos + i * plan->strip_size, SEEK_SET);
        if (fread(ptr[k + i], 1, bsize, fp) != static_cast<size_t>(bsize)) { rc = 1; break; }
      }
    if (rc) break;
    if (decode_stripes_impl(ext_of(plan), ptr.data(), 1, bsize, erasures)) { rc = 1; break; }
    for (int i = 0; i < k; ++i) {
      if (!missing[i]) continue;
      const long long bpos = apos + i * plan->strip_size;
      fseek(fd, bpos, SEEK_SET);
      // the last data strip is truncated to the file size (erasure_tools.c:576-582)
      const long long len = (i == k - 1 && bpos + bsize > fsize) ? fsize - bpos : bsize;
      if (len > 0 && fwrite(ptr[i], 1, len, fd) != static_cast<size_t>(len)) rc = 1;
    }
  }
  fclose(fd);
  fclose(fp);
  return rc;
}


int lsec_prepare_decode(lio_erasure_plan_t *plan, const int *erasures) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  std::vector<int> ids;
  const int pr = parse_erasures(plan, erasures, ids);
  if (pr != 0) return pr < 0 ? -1 : 0;
  CodingJob job;
  if (decode_job(e, ids, &job)) return -1;
  (void)lsec::jit::wait(job.image, 30000);  // a wide code's XOR network, if it has one
  return 0;
}

int lsec_prepare_encode(lio_erasure_plan_t *plan) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  CodingJob job;
  if (encode_job(e, &job)) return -1;
  (void)lsec::jit::wait(job.image, 30000);
  return 0;
}

int lsec_plan_jit(lio_erasure_plan_t *plan, const int *erasures) {
  PlanExt *e = ext_of(plan);
  if (!e) return 0;
  const int kind = kernel_kind(e->pub.method, e->pub.w);
  if (kind == KBYTEWISE ? lsec::bytewise_variant() != 0
                        : (kind == KWORDWISE || kind == KBITMATRIX || kind == KBITSLICEDW || kind == KBITSLICED)
                            ? lsec::bitsliced_variant() != 0
                            : true)
    return 0;
  CodingJob job;
  std::vector<int> ids;
  if (erasures ? parse_erasures(plan, erasures, ids) != 0 || decode_job(e, ids, &job) : encode_job(e, &job)) return 0;
  // Cauchy w = 8 shapes the bit-sliced kernel serves (at the plan's chunk size) run no network
  if (kind == KBITSLICED && plan->w == 8 && cauchy8_bitsliced_dw(plan->data_strips, job.R, plan->strip_size) > 0) return 0;
  return lsec::jit::ready(job.image, job.R, plan->data_strips) != nullptr ? 1 : 0;
}

int lsec_plan_kernel(lio_erasure_plan_t *plan) { return plan ? kernel_kind(plan->method, plan->w) : 0; }

void lsec_set_kernel_variant(int bytewise_variant, int bitsliced_variant) {
  lsec::set_kernel_variant(bytewise_variant, bitsliced_variant);
}

void lsec_set_tile_sharing(int mode) { lsec::set_tile_mode(mode); }

int lsec_tile_sharing(void) { return lsec::tile_mode(); }

// Test hook, not in include/: device buffer of n u64 for the bytewise kernels' per-workgroup end
// times (s_memrealtime) in the following launches, or NULL to stop (tools/xcd_stamps.py).
void lsec_test_set_stamps(void *dev_buf, unsigned n) {
  lsec::set_launch_stamps(static_cast<unsigned long long *>(dev_buf), n);
}

// Test hook, not in include/: what the calling thread's last lsec_encode_dev / lsec_decode_dev
// launched -- bit 0 a compiled XOR / GF(2^w) network, bit 1 a compiled packet network, bit 2 a
// generic kernel (a w = 16 / 32 network with a ragged tail: bits 0 and 2).  The bytes are the same
// on every path, so only this tells a test which one alignment and readiness picked.
int lsec_test_apply_path(void) { return tl_apply_path; }

// Test hook, not in include/: the kernel forms (ec_kernels.h, LaunchForm) that the calling thread's last
// lsec_check_dev, lsec_locate_dev, lsec_decode_dev_patterns, lsec_decode_dev_rotated,
// lsec_check_dev_rotated, lsec_locate_dev_rotated, lsec_update_dev, lsec_encode_dev_rotated,
// lsec_update_dev_rotated, lsec_update_dev_masked(_rotated), lsec_decode_magic_dev_patterns / _rotated,
// lsec_check_magic_dev(_rotated) or lsec_encode_magic_dev_rotated launched, in order: a locate with repair its
// patterned decode too, a split call every launch; the finalize launch, which has one form, is not
// among them.  forms: 8 ints each (family, bit-sliced, R, KC, IT, VW, BF, DW).  Returns the number
// of launches; at most min(that, max_forms, 16) are written.
int lsec_test_launch_record(int *forms, int max_forms) {
  lsec::LaunchForm rec[lsec::kLaunchRecordMax];
  const int n = lsec::launch_record(rec, lsec::kLaunchRecordMax);
  for (int i = 0; forms && i < n && i < max_forms && i < lsec::kLaunchRecordMax; ++i) {
    const int v[8] = {rec[i].family, rec[i].sliced, rec[i].R, rec[i].KC, rec[i].IT, rec[i].VW, rec[i].BF, rec[i].DW};
    std::memcpy(forms + 8 * i, v, sizeof(v));
  }
  return n;
}

// Test hook, not in include/ (no GPU): the form a launch of `family` (1 check, 2 locate, 3 rotated
// check, 4 rotated locate, 5 patterned decode, 6 rotated repair, 7 parity update, 8 rotated encode, 9 rotated
// parity update) takes for a plan of kernel 1
// (bytewise) or 2 (bit-sliced) with K inputs and R rows (patterned: the table's largest erasure
// count) at that packet and chunk size, as 8 ints.  It asks the functions the dispatch calls
// (cauchy8_bitsliced_dw here, lsec::predict_launch for the rest).  0, or -1 with a message.
int lsec_test_predict_form(int family, int plan_kernel, int K, int R, int packet, long long block_size, int *form) {
  if (!form) return fail("lsec_test_predict_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED) return fail("lsec_test_predict_form: plan kernel %d", plan_kernel);
  const bool sliced = plan_kernel == KBITSLICED;
  lsec::LaunchForm f;
  if (!lsec::predict_launch(family, sliced, K, R, packet, sliced ? cauchy8_bitsliced_dw(K, R, block_size) : 0, &f))
    return fail("lsec_test_predict_form: no kernel of family %d for K=%d R=%d packet=%d", family, K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): lsec_test_predict_form for the masked update (family 10 of the
// launch record, which that hook keeps refusing): the form lsec_update_dev_masked and
// lsec_update_dev_masked_rotated launch for a plan of kernel 1 or 2 with K columns and R rows, from
// the functions the dispatch calls (cauchy8_bitsliced_dw here, lsec::predict_masked_launch).
int lsec_test_predict_masked_form(int plan_kernel, int K, int R, int packet, long long block_size, int *form) {
  if (!form) return fail("lsec_test_predict_masked_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_masked_form: plan kernel %d", plan_kernel);
  const bool sliced = plan_kernel == KBITSLICED;
  lsec::LaunchForm f;
  if (!lsec::predict_masked_launch(sliced, K, R, packet, sliced ? cauchy8_bitsliced_dw(K, R, block_size) : 0, &f))
    return fail("lsec_test_predict_masked_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): lsec_test_predict_masked_form for the masked update that keeps the stripe
// magics (family 11 of the launch record): the form lsec_update_magic_dev_masked and
// lsec_update_magic_dev_masked_rotated launch, from the functions the dispatch calls.
int lsec_test_predict_masked_magic_form(int plan_kernel, int K, int R, int packet, long long block_size, int *form) {
  if (!form) return fail("lsec_test_predict_masked_magic_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_masked_magic_form: plan kernel %d", plan_kernel);
  const bool sliced = plan_kernel == KBITSLICED;
  lsec::LaunchForm f;
  if (!lsec::predict_masked_magic_launch(sliced, K, R, packet, sliced ? cauchy8_bitsliced_dw(K, R, block_size) : 0, &f))
    return fail("lsec_test_predict_masked_magic_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): the form (family 16, or 17 with `rotated`, of the launch record)
// lsec_search_dev_patterns and lsec_search_dev_patterns_rotated launch for a plan of kernel 1 or 2 with K inputs and a
// table of at most R erasures per pattern (R >= 1), from the function the dispatch calls.
int lsec_test_predict_search_form(int rotated, int plan_kernel, int K, int R, int packet, int *form) {
  if (!form) return fail("lsec_test_predict_search_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED) return fail("lsec_test_predict_search_form: plan kernel %d", plan_kernel);
  lsec::LaunchForm f;
  if (!lsec::predict_pattern_search_launch(rotated != 0, plan_kernel == KBITSLICED, K, R, packet, &f))
    return fail("lsec_test_predict_search_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/: the search's tile order (cand_outer 0: the candidate innermost, the default; 1: the
// piece of the chunk innermost) and load kind (plain_loads 0: non-temporal; 1: plain, the default) for A/B runs in
// one process (tools/search_ab.py).  The results do not depend on either.
void lsec_test_set_search_form(int cand_outer, int plain_loads) {
  g_search_cand_outer.store(cand_outer ? 1 : 0, std::memory_order_relaxed);
  g_search_plain_loads.store(plain_loads ? 1 : 0, std::memory_order_relaxed);
}

// Test hook, not in include/: the blank scan's load kind (plain_loads 0: non-temporal; 1: plain) and its tile (steps:
// 16-byte steps per lane, 2 or 4; anything else: 2) for A/B runs in one process (tools/vote_ab.py).  The results do
// not depend on either.
void lsec_test_set_vote_form(int plain_loads, int steps) {
  g_vote_plain_loads.store(plain_loads ? 1 : 0, std::memory_order_relaxed);
  g_vote_steps.store(steps == 4 ? 4 : 2, std::memory_order_relaxed);
}

// Test hook, not in include/ (no GPU): the form (family 12 of the launch record) lsec_decode_magic_dev_patterns and
// lsec_decode_magic_dev_rotated launch for a plan of kernel 1 or 2 with K inputs and a table of at most R erasures
// per pattern (a table of empty patterns launches the one-row form), from the function the dispatch calls.
int lsec_test_predict_pattern_magic_form(int plan_kernel, int K, int R, int packet, int *form) {
  if (!form) return fail("lsec_test_predict_pattern_magic_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_pattern_magic_form: plan kernel %d", plan_kernel);
  lsec::LaunchForm f;
  if (!lsec::predict_pattern_magic_launch(plan_kernel == KBITSLICED, K, R, packet, &f))
    return fail("lsec_test_predict_pattern_magic_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): the form (family 18 of the launch record) lsec_decode_magic_dev_patterns_rotated
// launches for a plan of kernel 1 or 2 with K inputs and a table of at most R erasures per pattern (a table of empty
// patterns launches the one-row form), from the function the dispatch calls.
int lsec_test_predict_pattern_magic_rot_form(int plan_kernel, int K, int R, int packet, int *form) {
  if (!form) return fail("lsec_test_predict_pattern_magic_rot_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_pattern_magic_rot_form: plan kernel %d", plan_kernel);
  lsec::LaunchForm f;
  if (!lsec::predict_pattern_magic_rot_launch(plan_kernel == KBITSLICED, K, R, packet, &f))
    return fail("lsec_test_predict_pattern_magic_rot_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): the form (family 13 of the launch record, 14 with `rotated`) lsec_check_magic_dev
// and lsec_check_magic_dev_rotated launch for a plan of kernel 1 or 2 with K inputs and R rows at that packet and
// chunk size, from the functions the dispatch calls (cauchy8_bitsliced_dw here, lsec::predict_check_magic_launch).
int lsec_test_predict_check_magic_form(int rotated, int plan_kernel, int K, int R, int packet, long long block_size, int *form) {
  if (!form) return fail("lsec_test_predict_check_magic_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_check_magic_form: plan kernel %d", plan_kernel);
  const bool sliced = plan_kernel == KBITSLICED;
  lsec::LaunchForm f;
  if (!lsec::predict_check_magic_launch(rotated != 0, sliced, K, R, packet, sliced ? cauchy8_bitsliced_dw(K, R, block_size) : 0, &f))
    return fail("lsec_test_predict_check_magic_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): the form (family 15 of the launch record) lsec_encode_magic_dev_rotated launches
// for a plan of kernel 1 or 2 with K inputs and R rows at that packet and chunk size, from the functions the dispatch
// calls (cauchy8_bitsliced_dw here, lsec::predict_encode_magic_launch).
int lsec_test_predict_encode_magic_form(int plan_kernel, int K, int R, int packet, long long block_size, int *form) {
  if (!form) return fail("lsec_test_predict_encode_magic_form: NULL output");
  if (plan_kernel != KBYTEWISE && plan_kernel != KBITSLICED)
    return fail("lsec_test_predict_encode_magic_form: plan kernel %d", plan_kernel);
  const bool sliced = plan_kernel == KBITSLICED;
  lsec::LaunchForm f;
  if (!lsec::predict_encode_magic_launch(sliced, K, R, packet, sliced ? cauchy8_bitsliced_dw(K, R, block_size) : 0, &f))
    return fail("lsec_test_predict_encode_magic_form: no kernel for K=%d R=%d packet=%d", K, R, packet);
  const int v[8] = {f.family, f.sliced, f.R, f.KC, f.IT, f.VW, f.BF, f.DW};
  std::memcpy(form, v, sizeof(v));
  return 0;
}

// Test hook, not in include/ (no GPU): what the magic form adds to entry pattern_id of the table of
// lsec_test_pattern_table (same arguments): *nout its erasure count (0: the checksum-only path; -1: a rotation that
// cannot occur), in_sel[0..k) the shard indices it loads as inputs (for nout 0 too: the data chunks),
// out_sel[0..nout), and unused[0..return value) the survivors it loads for the checksum alone.  Returns their
// count, or -1 with a message.
int lsec_test_pattern_unused(lio_erasure_plan_t *plan, const int *patterns, int npatterns, const int *lost, int n_shift,
                             int pattern_id, int *nout, int *in_sel, int *out_sel, int *unused) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  if (!nout || !in_sel || !out_sel || !unused) return fail("lsec_test_pattern_unused: NULL output");
  if (decode_magic_limits(plan, "lsec_test_pattern_unused")) return -1;
  PatternTable tab;
  if (build_pattern_table(e, patterns, npatterns, lost, n_shift, tab)) return -1;
  if (pattern_id < 0 || pattern_id >= static_cast<int>(tab.recs.size()))
    return fail("lsec_test_pattern_unused: entry %d outside 0..%zu", pattern_id, tab.recs.size() - 1);
  const lsec::PatRecord &rec = tab.recs[pattern_id];
  const lsec::PatUnused &un = tab.unused[pattern_id];
  *nout = tab.reachable[pattern_id] ? static_cast<int>(rec.nout) : -1;
  for (int j = 0; j < plan->data_strips; ++j) in_sel[j] = static_cast<int>(rec.in_sel[j]);
  for (uint32_t r = 0; r < rec.nout; ++r) out_sel[r] = static_cast<int>(rec.out_sel[r]);
  for (uint32_t u = 0; u < un.n; ++u) unused[u] = static_cast<int>(un.sel[u]);
  return static_cast<int>(un.n);
}

// Test hook, not in include/ (no GPU): the K that have fixed-K forms (LSEC_FIXED_K), ascending
int lsec_test_fixed_k(int *out, int max) { return lsec::fixed_k_list(out, max); }

namespace {
int put_apply_forms(const lsec::ApplyForm *f, int n, int *forms, int max_forms) {
  for (int i = 0; forms && i < n && i < max_forms; ++i) {
    const int v[lsec::kApplyFormInts] = {f[i].kind, f[i].R, f[i].KC, f[i].IT, f[i].VW, f[i].BF, f[i].DW, f[i].w, f[i].acc, f[i].magic, f[i].sub, f[i].loop};
    std::memcpy(forms + lsec::kApplyFormInts * i, v, sizeof(v));
  }
  return n;
}
}  // namespace

// Test hook, not in include/: the kernels (ec_kernels.h, ApplyForm) that the calling thread's last lsec_encode_dev,
// lsec_decode_dev or lsec_encode_magic_dev launched through the table dispatch, in order: input groups x row
// launches x stripe ranges.  A compiled network's launch is not among them (lsec_test_apply_path tells), nor is
// the magic pass of a two-pass lsec_encode_magic_dev.  forms: 12 ints each (kind, R, KC, IT, VW, BF, DW, w,
// accumulate, fused magic, sub, loop).  Returns the number of launches; at most min(that, max_forms, 64) are written.
int lsec_test_apply_record(int *forms, int max_forms) {
  lsec::ApplyForm rec[lsec::kApplyRecordMax];
  const int n = lsec::apply_record(rec, lsec::kApplyRecordMax);
  put_apply_forms(rec, std::min(n, lsec::kApplyRecordMax), forms, max_forms);
  return n;
}

// Test hook, not in include/ (no GPU): the forms, as lsec_test_apply_record lists them, that one unsplit call of a
// K x R matrix of kernel `kind` (1-5) launches at word size w, that packet and chunk size under the two variant
// values of lsec_set_kernel_variant, while no network is ready; fused_magic: lsec_encode_magic_dev.  row_ones:
// R bytes, nonzero where the row is all ones (NULL: none).  It asks the functions the calls themselves go
// through (predict_apply).  Returns the number of launches (at most max_forms are written), or -1 with a message.
int lsec_test_predict_apply(int kind, int K, int R, int w, int packet, long long block_size, int fused_magic, int bw_variant,
                            int bs_variant, const unsigned char *row_ones, int *forms, int max_forms) {
  std::vector<lsec::ApplyForm> f;
  if (predict_apply(kind, K, R, w, packet, block_size, fused_magic != 0, bw_variant, bs_variant, row_ones, f)) return -1;
  return put_apply_forms(f.data(), static_cast<int>(f.size()), forms, max_forms);
}

// Test hook, not in include/ (no GPU): the form one launch of K inputs and R rows takes (lsec::predict_apply_launch),
// unsplit: lsec_test_predict_apply cuts a call into the launches enqueue_apply makes, so a kernel that is compiled
// for more rows than a launch ever gets is named by this hook alone.  0, or -1 where the launch would be refused.
int lsec_test_predict_apply_launch(int kind, int K, int R, int w, int packet, int accumulate, int fused_magic, int dw_pref,
                                   int bw_variant, int bs_variant, int first_row_ones, int *form) {
  if (!form) return fail("lsec_test_predict_apply_launch: NULL output");
  lsec::ApplyForm f;
  if (!lsec::predict_apply_launch(kind, K, R, w, packet, accumulate != 0, fused_magic != 0, dw_pref, bw_variant, bs_variant,
                                  first_row_ones != 0, &f))
    return fail("lsec_test_predict_apply_launch: no kernel of kind %d for K=%d R=%d w=%d packet=%d", kind, K, R, w, packet);
  put_apply_forms(&f, 1, form, 1);
  return 0;
}

// Test hook, not in include/ (no GPU): lsec_test_predict_apply for a plan's own matrices under the variant
// values in force -- the encode (erasures NULL; fused_magic: lsec_encode_magic_dev) or the decode of a
// -1 terminated erasure list, whose kernel kind, row count and rows of ones come from the host side of the
// plan's decode cache.  0 launches where the call has nothing to do.
int lsec_test_predict_apply_plan(lio_erasure_plan_t *plan, const int *erasures, long long block_size, int fused_magic,
                                 int *forms, int max_forms) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  if (ensure_coding(e)) return -1;
  const int k = plan->data_strips;
  int kind = kernel_kind(plan->method, plan->w), R = 0;
  const uint8_t *rows = nullptr;
  if (!erasures) {
    R = encode_rows(e);
    if (!uses_u32_image(kind)) rows = e->impl->coding.data();
  } else {
    std::vector<int> ids;
    const int pr = parse_erasures(plan, erasures, ids);
    if (pr < 0) return -1;
    if (pr == 1 || (plan->method == RAID4 && ids[0] >= k)) return 0;
    DecodeEntry *ent = nullptr;
    {
      std::lock_guard<std::mutex> lk(e->impl->mu);
      if (decode_host_locked(e, ids, &ent)) return -1;
    }
    const bool field = kind == KBITSLICED || kind == KWORDWISE || kind == KBITSLICEDW;
    if (field && ent->xor_only) kind = KBYTEWISE;  // (decode_job)
    R = static_cast<int>(ent->dp.erased.size());
    if (!uses_u32_image(kind)) rows = ent->dp.rows.data();
  }
  std::vector<unsigned char> ones(R, 0);
  for (int r = 0; rows && r < R; ++r) ones[r] = apply_first_row_ones(rows, k, 0, r) ? 1 : 0;
  std::vector<lsec::ApplyForm> f;
  if (predict_apply(kind, k, R, plan->w, plan->packet_size, block_size, fused_magic != 0, lsec::bytewise_variant(),
                    lsec::bitsliced_variant(), ones.data(), f))
    return -1;
  return put_apply_forms(f.data(), static_cast<int>(f.size()), forms, max_forms);
}

// Test hook, not in include/: while `on` is nonzero no compiled network counts as ready, so every call runs the
// table kernels under the automatic policy, as a plan's first calls do before its network is compiled.  It reads
// an atomic per call: no compile timing and no environment variable is involved.
void lsec_test_hold_networks(int on) { g_hold_networks.store(on ? 1 : 0, std::memory_order_relaxed); }

// Test hook, not in include/: 1 = Cauchy at w = 8 on its compiled packet network wherever one exists,
// 0 = by shape (cauchy8_bitsliced_dw, the default).
void lsec_test_set_cauchy8_policy(int mode) { g_c8_policy.store(mode == 1 ? 1 : 0, std::memory_order_relaxed); }

// Test hook, not in include/: the XCD tile phase for the following launches, bit 0 the tile loops,
// bit 1 the compiled networks (lsec::tile_phase_on; LSEC_TILE_PHASE sets the start value, 1), for
// A/B runs in one allocation.
void lsec_test_set_tile_phase(int mode) { lsec::set_tile_phase(mode); }

// Test hook, not in include/: a patterned call (and lsec_update_dev, lsec_encode_dev_rotated,
// lsec_update_dev_rotated, lsec_update_dev_masked(_rotated), lsec_decode_magic_dev_patterns / _rotated and
// lsec_check_magic_dev(_rotated)) launches at most `stripes` stripes at a time (0, the default: only the 32-bit tile limit splits), so a small batch exercises
// the split.
void lsec_test_set_pattern_split(int stripes) { g_pattern_split.store(std::max(0, stripes), std::memory_order_relaxed); }

// Test hook, not in include/ (no GPU): entry pattern_id of the table the host builds for
// lsec_decode_dev_patterns (patterns != NULL) or lsec_decode_dev_rotated (patterns NULL: lost,
// n_shift; pattern_id is the rotation).  *nout = its erasure count (-1: a rotation that cannot
// occur), in_sel[0..k) and out_sel[0..nout) its shard indices, coef[nout * k] its decode rows.
// 0, or -1 with a message.
int lsec_test_pattern_table(lio_erasure_plan_t *plan, const int *patterns, int npatterns, const int *lost, int n_shift,
                            int pattern_id, int *nout, int *in_sel, int *out_sel, int *coef) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  if (!nout || !in_sel || !out_sel || !coef) return fail("lsec_test_pattern_table: NULL output");
  PatternTable tab;
  if (build_pattern_table(e, patterns, npatterns, lost, n_shift, tab)) return -1;
  if (pattern_id < 0 || pattern_id >= static_cast<int>(tab.recs.size()))
    return fail("lsec_test_pattern_table: entry %d outside 0..%zu", pattern_id, tab.recs.size() - 1);
  const lsec::PatRecord &rec = tab.recs[pattern_id];
  const int k = plan->data_strips;
  *nout = tab.reachable[pattern_id] ? static_cast<int>(rec.nout) : -1;
  for (int j = 0; j < k; ++j) in_sel[j] = rec.nout ? static_cast<int>(rec.in_sel[j]) : -1;
  for (uint32_t r = 0; r < rec.nout; ++r) {
    out_sel[r] = static_cast<int>(rec.out_sel[r]);
    for (int j = 0; j < k; ++j) coef[r * k + j] = static_cast<int>(tab.cells[rec.cells_off + r * k + j].coef);
  }
  // the rows past the entry's own count must be zero cells
  for (int r = static_cast<int>(rec.nout); rec.nout && r < tab.rmax; ++r)
    for (int j = 0; j < k; ++j)
      if (tab.cells[rec.cells_off + static_cast<size_t>(r) * k + j].coef != 0 ||
          tab.cells[rec.cells_off + static_cast<size_t>(r) * k + j].ta_lo != 0)
        return fail("lsec_test_pattern_table: entry %d row %d is not zero", pattern_id, r);
  return 0;
}

// Test hook, not in include/ (no GPU): Q[r][j] = g[r+1][j] / g[0][j] of the host ratio image that
// lsec_locate_dev uploads (0 <= r < m-1, 0 <= j < k), or -1 with a message.
int lsec_test_locate_ratio(lio_erasure_plan_t *plan, int r, int j) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  const int kind = kernel_kind(plan->method, plan->w);
  if (kind != KBYTEWISE && kind != KBITSLICED) return fail("lsec_test_locate_ratio: plan kernel %d", kind);
  if (plan->parity_strips < 2) return fail("lsec_test_locate_ratio: m=%d", plan->parity_strips);
  const lsec::gf8::Mat *q = nullptr;
  if (locate_ratio(e, &q)) return -1;
  if (r < 0 || r >= plan->parity_strips - 1 || j < 0 || j >= plan->data_strips)
    return fail("lsec_test_locate_ratio: [%d][%d] outside %d x %d", r, j, plan->parity_strips - 1, plan->data_strips);
  return (*q)[static_cast<size_t>(r) * plan->data_strips + j];
}

// Test hook, not in include/: the device allocations the plan owns now, summed over every DevImage
// (an image counts once per device it was uploaded to), or -1 with a message.
int lsec_test_plan_images(lio_erasure_plan_t *plan) {
  PlanExt *e = ext_of(plan);
  if (!e) return fail("not an lstore_ec plan");
  std::lock_guard<std::mutex> lk(e->impl->mu);
  size_t n = 0;
  e->impl->for_each_image([&](const DevImage &img) { n += img.count(); });
  return static_cast<int>(n);
}

// Test hook, not in include/: the rotation of a rotated call's first stripe, as the call computes it
int lsec_test_pattern_rot0(int n, int n_shift, long long first_stripe) {
  if (n < 1 || n_shift < 0 || first_stripe < 0) return fail("lsec_test_pattern_rot0: n >= 1, n_shift >= 0, first_stripe >= 0");
  return static_cast<int>(pattern_rot0(n, n_shift, first_stripe));
}


// Self-test of the bitmatrix decode planner (test hook, not in include/; no GPU): for the
// liberation-family plan (method, k, w) with m = 2, make_bit_decode's masks must equal those of
// the whole-bitmatrix inversion (make_bit_decode_dense) for every erasure pattern of one and two
// devices.  Returns the number of patterns compared, or -1 with a message.
int lsec_selftest_bit_decode(int method, int k, int w) {
  std::vector<int> bm = method == LIBERATION   ? lsec::gf8::liberation_bitmatrix(k, w)
                        : method == BLAUM_ROTH ? lsec::gf8::blaum_roth_bitmatrix(k, w)
                        : method == LIBER8TION ? lsec::gf8::liber8tion_bitmatrix(k)
                                               : std::vector<int>();
  if (bm.empty()) return fail("lsec_selftest_bit_decode: no %d bitmatrix for k=%d w=%d", method, k, w);
  const int m = 2;
  int n = 0;
  for (int a = 0; a < k + m; ++a)
    for (int b = a; b < k + m; ++b) {
      std::vector<int> ids = a == b ? std::vector<int>{a} : std::vector<int>{a, b};
      lsec::gf8::DecodePlan p1, p2;
      std::vector<uint32_t> m1, m2;
      const bool ok1 = lsec::gf8::make_bit_decode(k, m, w, bm, ids, p1, m1);
      const bool ok2 = lsec::gf8::make_bit_decode_dense(k, m, w, bm, ids, p2, m2);
      if (ok1 != ok2 || p1.survivors != p2.survivors || p1.erased != p2.erased || m1 != m2)
        return fail("lsec_selftest_bit_decode: erasures {%d, %d} differ (ok %d/%d)", a, b, ok1, ok2);
      ++n;
    }
  return n;
}

}  // extern "C"
