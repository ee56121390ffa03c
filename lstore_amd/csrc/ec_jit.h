// ec_jit.h -- the run-time compiled networks of wide matrix and bitmatrix codes: binding a device
// image to its network, and launching it (ec_jit.cpp; what a network is: ec_netgen.h).
// Internal to liblstore_ec.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ec_kernels.h"
#include "ec_netgen.h"

namespace lsec {
namespace jit {

// Associate a device coefficient image with its matrix and start compiling that matrix's
// network in the background (once per matrix per process).  unbind before the image is freed.
void bind(const void *image, const uint8_t *mat, int R, int K);
void bind_w(const void *image, const uint32_t *mat, int R, int K, int w);  // w = 16 / 32
// bind a bitmatrix image (ungrouped row masks, K <= 32) to its packet network; the lane width
// follows the packet size
void bind_pkt(const void *image, const uint32_t *masks, int R, int K, int w, int packet);
// the same for an R x K GF(2^w) coefficient matrix in Cauchy's packet layout (w = 8 / 16 / 32)
void bind_pkt_field(const void *image, const uint32_t *coef, int R, int K, int w, int packet);
void unbind(const void *image);
// Block until the image's network is compiled (or failed, or timeout): 1 ready, 0 otherwise
// (also 0 when the image has no network).
int wait(const void *image, int timeout_ms);
// The compiled network for `image` on the current device, or nullptr (not bound / not ready).
hipFunction_t ready(const void *image, int R, int K);
// out[r] = sum_j A[r][j] in[j] for every stripe (same shard addressing as ApplyArgs); at
// w = 16 / 32 over the first size / gfw_tile(w, R) whole tiles of every shard only.
hipError_t launch(hipFunction_t fn, int R, int K, const ShardRef *in, const ShardRef *out, int nstripes, int64_t size,
                  hipStream_t st, int w = 8);
// out[r] packets = the bitmatrix rows' XORs of the input packets, every stripe; the shard bases
// and strides must be aligned to the lane width (pkt_aligned)
hipError_t launch_pkt(hipFunction_t fn, int R, int K, const ShardRef *in, const ShardRef *out, int nstripes, int64_t size,
                      int packet, int w, hipStream_t st);
bool pkt_aligned(const ShardRef *in, int K, const ShardRef *out, int R, int w, int packet);

}  // namespace jit
}  // namespace lsec
