// The host-fed input path (gfx950 only): one packed record per step, shipped by ONE DMA, unpacked on the device.
//   ingest_unpack_kernel   stands where the reference converts the host arrays of a control cycle into the tensors PAN.forward
//                          takes: np_to_tensor at neupan/neupan.py:121 (the nominal / reference tensors) and :123-127 (the
//                          obstacle points and their velocities)
// The record (include/neupan_amd.h, "packed input record") carries ragged clouds back to back; the kernel writes the padded
// [B][2][n_stride] arrays the selection kernel reads.  It is what separates the DMA target from the buffers a running step
// reads: the upload of cycle i+1 lands in a spare record while cycle i computes, and this launch -- stream-ordered behind
// cycle i's kernels -- moves it into place.  Pure data movement: words are copied as 32-bit integers, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace {

constexpr int INGEST_THREADS = 256;
constexpr size_t INGEST_ALIGN = 256;      // every section of a record starts on a 256-byte boundary

struct IngestLayout {
  size_t n_points, cloud_off, nom_s, nom_u, ref_s, ref_us, cloud, total;     // byte offsets, worst-case bytes
};

inline size_t align_up(size_t v) { return (v + INGEST_ALIGN - 1) / INGEST_ALIGN * INGEST_ALIGN; }

inline IngestLayout ingest_layout(int B, int T, int n_stride, int with_vel) {
  IngestLayout L;
  size_t o = 0, b = (size_t)B;
  L.n_points = o;  o = align_up(o + b * 4);
  L.cloud_off = o; o = align_up(o + b * 4);
  L.nom_s = o;     o = align_up(o + b * 3 * (T + 1) * 4);
  L.nom_u = o;     o = align_up(o + b * 2 * T * 4);
  L.ref_s = o;     o = align_up(o + b * 3 * (T + 1) * 4);
  L.ref_us = o;    o = align_up(o + b * T * 4);
  L.cloud = o;     o = align_up(o + b * (size_t)n_stride * (with_vel ? 4 : 2) * 4);
  L.total = o;
  return L;
}

// `n` words from src to dst by the threads of slice `part` of `parts` (all arguments the same in every lane of the block).
// 16-byte accesses where BOTH addresses allow them, else coalesced 4-byte ones: a cloud starts wherever the prefix sum of
// the scenes in front of it put it.
__device__ inline void copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int n, int part, int parts) {
  const int tid = part * INGEST_THREADS + (int)threadIdx.x, step = parts * INGEST_THREADS;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    const int n4 = n >> 2;
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
    for (int i = tid; i < n4; i += step) d4[i] = s4[i];
    for (int i = (n4 << 2) + tid; i < n; i += step) dst[i] = src[i];
  } else {
    for (int i = tid; i < n; i += step) dst[i] = src[i];
  }
}

// grid (batch, parts): block (b, p) moves slice p of scene b's cloud; the blocks p == 0 also move the scene's dense rows and
// its header.  The header (n_b, offset) is addressed by blockIdx alone: scalar loads, one decision per block, no divergence.
// A scene whose header does not describe a cloud inside the record's cloud section is planned WITHOUT points
// (n_points = 0) and reported in status: (count of such scenes, smallest such index); nothing of it is read.
__global__ __launch_bounds__(INGEST_THREADS) void ingest_unpack_kernel(
    int T, int n_stride, int comps, IngestLayout L, long long cloud_words, const unsigned char* __restrict__ rec,
    uint32_t* __restrict__ nom_s, uint32_t* __restrict__ nom_u, uint32_t* __restrict__ ref_s, uint32_t* __restrict__ ref_us,
    uint32_t* __restrict__ points, uint32_t* __restrict__ velocities, int* __restrict__ n_points, int* __restrict__ status) {
  const int b = (int)blockIdx.x, part = (int)blockIdx.y, parts = (int)gridDim.y;
  const int n = reinterpret_cast<const int*>(rec + L.n_points)[b];
  const int off = reinterpret_cast<const int*>(rec + L.cloud_off)[b];
  // (n == 0 owns no words: any offset is fine)
  const bool ok = n == 0 || (n > 0 && n <= n_stride && off >= 0 && (long long)off + (long long)comps * n <= cloud_words);
  if (part == 0) {
    const int ns = 3 * (T + 1), nu = 2 * T;
    copy_words(nom_s + (size_t)b * ns, reinterpret_cast<const uint32_t*>(rec + L.nom_s) + (size_t)b * ns, ns, 0, 1);
    copy_words(nom_u + (size_t)b * nu, reinterpret_cast<const uint32_t*>(rec + L.nom_u) + (size_t)b * nu, nu, 0, 1);
    copy_words(ref_s + (size_t)b * ns, reinterpret_cast<const uint32_t*>(rec + L.ref_s) + (size_t)b * ns, ns, 0, 1);
    copy_words(ref_us + (size_t)b * T, reinterpret_cast<const uint32_t*>(rec + L.ref_us) + (size_t)b * T, T, 0, 1);
    if (threadIdx.x == 0) {
      n_points[b] = ok ? n : 0;
      if (!ok) {
        atomicAdd(&status[0], 1);
        atomicMin(&status[1], b);
      }
    }
  }
  if (!ok || n == 0) return;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(rec + L.cloud) + off;
  for (int c = 0; c < comps; ++c) {            // x, y (, vx, vy): n words each, columns [n, n_stride) are not written
    uint32_t* __restrict__ dst = (c < 2 ? points : velocities) + ((size_t)b * 2 + (c & 1)) * (size_t)n_stride;
    copy_words(dst, src + (size_t)c * n, n, part, parts);
  }
}

}  // namespace

// out[0..n), n <= 8: byte offsets of n_points, cloud_off, nom_s, nom_u, ref_s, ref_us, the cloud section; worst-case bytes.
int npa_ingest_offsets(int batch, int T, int n_stride, int with_vel, size_t* out, int n) {
  // (cloud_off is an int32 word offset: the cloud section must stay below 2^31 words)
  if ((size_t)batch * (size_t)n_stride * (with_vel ? 4 : 2) >= ((size_t)1 << 31)) return -1;
  const IngestLayout L = ingest_layout(batch, T, n_stride, with_vel);
  const size_t v[8] = {L.n_points, L.cloud_off, L.nom_s, L.nom_u, L.ref_s, L.ref_us, L.cloud, L.total};
  for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
  return 0;
}

hipError_t npa_launch_ingest_unpack(int batch, int T, int n_stride, int with_vel, const void* record,
                                               size_t record_bytes, float* nom_s, float* nom_u, float* ref_s, float* ref_us,
                                               float* points, float* velocities, int* n_points, int* status,
                                               hipStream_t stream) {
  const IngestLayout L = ingest_layout(batch, T, n_stride, with_vel);
  // the caller (npa_ingest_unpack) has checked L.cloud <= record_bytes <= L.total: the header and the dense sections are inside
  const long long cloud_words = (long long)((record_bytes - L.cloud) / 4);
  int parts = (n_stride + 1023) / 1024;        // one block per scene up to 1024 points, more for long clouds
  parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
  auto u = [](float* p) { return reinterpret_cast<uint32_t*>(p); };
  hipLaunchKernelGGL(ingest_unpack_kernel, dim3(batch, parts), dim3(INGEST_THREADS), 0, stream, T, n_stride,
                     with_vel ? 4 : 2, L, cloud_words, static_cast<const unsigned char*>(record), u(nom_s), u(nom_u), u(ref_s),
                     u(ref_us), u(points), u(velocities), n_points, status);
  return hipGetLastError();
}
