// restart_kernels.hpp -- the snapshot of a checkpoint: ONE launch walks a table of segments, copies each into the arena with 16-byte
// loads and stores and forms the two integer checksums of restart_file.hpp in the same pass, every element read once.  The same
// kernel without stores checks an arena that came from a file, and with source and destination exchanged scatters it into the
// fields.  No atomics: a lane sums in registers, a wave by shuffles, a block through LDS, and each block stores ONE pair of
// partial sums; the host adds the blocks of a member (integer sums mod 2^64: exact, whatever the order).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gb25 {

// A contiguous run of elements of one member: whole 16-byte vectors, then the bytes behind the last whole vector element by
// element (the segment's first block).  scalar != 0: source or a destination is off a 16-byte boundary (the second and third array
// of a contiguous triple against the arena, whose offsets are multiples of 16): the whole segment goes element by element.
struct RestartSeg {
  const unsigned char* src;
  unsigned char* dst;    // null: checksums only
  unsigned char* dst2;   // a second copy (the partner buffer of an alternating pair), or null
  unsigned long long bytes, elem0;   // elem0: index in the member of the segment's first element
  unsigned int block0, nblocks;      // its blocks: [block0, block0 + nblocks)
  unsigned int elem_bytes, member, scalar;
};

constexpr int kRestartThreads = 256;
constexpr int kRestartVectorsPerBlock = 2048;   // 32 KB per block: eight 16-byte vectors per lane
constexpr unsigned long long kRestartBlockBytes = 16ull * kRestartVectorsPerBlock;

__device__ inline unsigned long long restart_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_down((unsigned)v, off, 64), hi = __shfl_down((unsigned)(v >> 32), off, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// element-wise over the bytes [b0, b1) of the segment (multiples of the element size)
template <class U>
__device__ inline void restart_scalar_run(const RestartSeg& g, unsigned long long b0, unsigned long long b1, unsigned long long& s1,
                                          unsigned long long& s2) {
  const unsigned long long n0 = b0 / sizeof(U), n1 = b1 / sizeof(U);
  const U* s = reinterpret_cast<const U*>(g.src);
  U* d = reinterpret_cast<U*>(g.dst);
  U* d2 = reinterpret_cast<U*>(g.dst2);
  for (unsigned long long n = n0 + threadIdx.x; n < n1; n += kRestartThreads) {
    const U x = s[n];
    if (d) d[n] = x;
    if (d2) d2[n] = x;
    s1 += (unsigned long long)x;
    s2 += (g.elem0 + n + 1) * (unsigned long long)x;
  }
}

__global__ __launch_bounds__(kRestartThreads) void k_restart_pack(const RestartSeg* __restrict__ segs, int nsegs,
                                                                  unsigned long long* __restrict__ partials) {
  int q = 0;   // (a few dozen segments at the most; uniform over the block)
  while (q + 1 < nsegs && blockIdx.x >= segs[q + 1].block0) q++;
  const RestartSeg g = segs[q];
  const unsigned lb = blockIdx.x - g.block0;
  unsigned long long s1 = 0, s2 = 0;
  const unsigned long long nv = g.scalar ? 0 : g.bytes / 16, tail0 = 16 * nv;
  {
    const uint4* __restrict__ vs = reinterpret_cast<const uint4*>(g.src);
    uint4* vd = g.dst ? reinterpret_cast<uint4*>(g.dst) : nullptr;
    uint4* vd2 = g.dst2 ? reinterpret_cast<uint4*>(g.dst2) : nullptr;
    const unsigned long long v0 = (unsigned long long)lb * kRestartVectorsPerBlock;
    const unsigned long long v1 = v0 + kRestartVectorsPerBlock < nv ? v0 + kRestartVectorsPerBlock : nv;
#pragma unroll 4
    for (unsigned long long v = v0 + threadIdx.x; v < v1; v += kRestartThreads) {
      const uint4 x = vs[v];
      if (vd) vd[v] = x;
      if (vd2) vd2[v] = x;
      if (g.elem_bytes == 4) {
        const unsigned long long e = g.elem0 + 4 * v;
        s1 += (unsigned long long)x.x + x.y + x.z + x.w;
        s2 += (e + 1) * x.x + (e + 2) * x.y + (e + 3) * x.z + (e + 4) * x.w;
      } else {
        const unsigned long long e = g.elem0 + 2 * v;
        const unsigned long long a = ((unsigned long long)x.y << 32) | x.x, b = ((unsigned long long)x.w << 32) | x.z;
        s1 += a + b;
        s2 += (e + 1) * a + (e + 2) * b;
      }
    }
  }
  // what the vectors leave: the tail (the segment's first block), or a segment that goes element by element altogether
  if (g.scalar) {
    const unsigned long long b0 = (unsigned long long)lb * kRestartBlockBytes;
    const unsigned long long b1 = b0 + kRestartBlockBytes < g.bytes ? b0 + kRestartBlockBytes : g.bytes;
    if (g.elem_bytes == 4) restart_scalar_run<unsigned int>(g, b0, b1, s1, s2);
    else restart_scalar_run<unsigned long long>(g, b0, b1, s1, s2);
  } else if (lb == 0) {
    if (g.elem_bytes == 4) restart_scalar_run<unsigned int>(g, tail0, g.bytes, s1, s2);
    else restart_scalar_run<unsigned long long>(g, tail0, g.bytes, s1, s2);
  }
  __shared__ unsigned long long part[2][kRestartThreads / 64];
  s1 = restart_wave_sum(s1);
  s2 = restart_wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = s1; part[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t1 = 0, t2 = 0;
    for (int w = 0; w < kRestartThreads / 64; w++) { t1 += part[0][w]; t2 += part[1][w]; }
    partials[2 * (unsigned long long)blockIdx.x] = t1;
    partials[2 * (unsigned long long)blockIdx.x + 1] = t2;
  }
}

}  // namespace gb25
