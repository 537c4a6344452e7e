// segment_matmul_dev.h — the device code segment_matmul.hip and segment_matmul_grad_w.hip share:
// the LDS slab layout of an MFMA operand, the two ways a slab is staged (a source whose rows run
// along the contraction is copied, one whose rows run across it is transposed on the way in), the
// 16-byte loads with their zero-filled tails and the matrix instruction of each dtype.
//
// Operand layout.  v_mfma_f32_32x32x16_{bf16,f16} takes from lane l of each operand eight
// contraction-consecutive values of tile row l % 32 (half l / 32 of the 16), v_mfma_f32_32x32x2f32
// one value; D[i][j] has j = l % 32 and i = 8 * (reg / 4) + 4 * (l / 32) + reg % 4.  A slab is
// kSlabBytes bytes of contraction per tile row; lane half h owns bytes [64 h, 64 h + 64) of its
// row as four 16-byte chunks, and chunk c feeds one 16-bit MFMA or four f32 ones.  Both operands
// use the same (h, c, element) -> k map, so which k an instruction sees where does not matter.
//
// LDS: slab row j at j * kRowStride bytes (128 + 16 of padding), its 16-byte chunk q stored at
// position q ^ ((j >> 4) & 7).  The padding makes the ds_read_b128 of 16 consecutive rows hit 64
// distinct banks; the swizzle is constant over those 16 rows (so it costs the reads nothing) and
// spreads the transposing 4-byte writes of 16 column groups, which without it fall on two banks.
#ifndef OFX_SEGMENT_MATMUL_DEV_H_
#define OFX_SEGMENT_MATMUL_DEV_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "segment_matmul.h"

namespace ofx {
namespace segmm {

constexpr int kRowStride = kSlabBytes + 16;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int lds_chunk(int j, int q) {
  return j * kRowStride + ((q ^ ((j >> 4) & 7)) << 4);
}

template <typename T>
__device__ __forceinline__ uint32_t bits_of(T v) {
  if constexpr (sizeof(T) == 2)
    return (uint32_t)__builtin_bit_cast(uint16_t, v);
  else
    return __builtin_bit_cast(uint32_t, v);
}

// The 16 bytes at columns [j, j + VEC) of the row at p, of which `ncols` exist: one 16-byte load
// when `vec` (p + j is 16-byte aligned) and the chunk is whole, scalar loads and zeros else.  A
// NULL row is a zero row and loads nothing.
template <typename T>
__device__ __forceinline__ uint4 load_chunk(const T* __restrict__ p, int64_t j, int64_t ncols,
                                            bool vec) {
  constexpr int VEC = 16 / sizeof(T);
  uint4 out = {0u, 0u, 0u, 0u};
  if (p == nullptr || j >= ncols) return out;
  if (vec && j + VEC <= ncols) return *reinterpret_cast<const uint4*>(p + j);
  uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const uint32_t b = j + e < ncols ? bits_of(p[j + e]) : 0u;
    if constexpr (sizeof(T) == 2)
      d[e >> 1] |= b << ((e & 1) * 16);
    else
      d[e] = b;
  }
  out.x = d[0], out.y = d[1], out.z = d[2], out.w = d[3];
  return out;
}

// Stages the slab of a source whose rows run along the contraction (row(j): tile row j at the
// slab's first k, or NULL; `kvalid` k exist from there): 16-byte copies.
template <typename T, int NC, typename RowFn>
__device__ __forceinline__ void stage_rows(char* lds, RowFn&& row, int64_t kvalid, bool vec) {
  constexpr int VEC = 16 / sizeof(T);
  for (int it = threadIdx.x; it < NC * 8; it += kThreads) {
    const int q = it & 7, j = it >> 3;
    *reinterpret_cast<uint4*>(lds + lds_chunk(j, q)) = load_chunk<T>(row(j), q * VEC, kvalid, vec);
  }
}

// Stages the slab of a source whose rows run across the contraction (row(k): the slab's k-th row
// at tile column 0, or NULL; `ncols` tile columns exist), transposed: a thread loads 16 bytes of
// columns from one row (f32) or from two consecutive rows (16-bit, packed into one dword a
// column) and writes a dword to each column's slab row.
template <typename T, int NC, typename RowFn>
__device__ __forceinline__ void stage_transposed(char* lds, RowFn&& row, int64_t ncols, bool vec) {
  constexpr int VEC = 16 / sizeof(T), BK = kSlabBytes / sizeof(T);
  constexpr int KG = sizeof(T) == 2 ? 2 : 1;
  constexpr int JQ = NC / VEC;
  for (int it = threadIdx.x; it < (BK / KG) * JQ; it += kThreads) {
    const int jq = it % JQ, kg = it / JQ;
    const int j = jq * VEC;
    const uint4 lo = load_chunk<T>(row(kg * KG), j, ncols, vec);
    uint32_t d[VEC];
    if constexpr (KG == 2) {
      const uint4 hi = load_chunk<T>(row(kg * KG + 1), j, ncols, vec);
      const uint32_t a[4] = {lo.x, lo.y, lo.z, lo.w}, b[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int sh = (e & 1) * 16;
        d[e] = ((a[e >> 1] >> sh) & 0xffffu) | (((b[e >> 1] >> sh) & 0xffffu) << 16);
      }
    } else {
      d[0] = lo.x, d[1] = lo.y, d[2] = lo.z, d[3] = lo.w;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      *reinterpret_cast<uint32_t*>(lds + lds_chunk(j + e, kg >> 2) + ((kg & 3) << 2)) = d[e];
  }
}

// Chunk c of lane half h of slab row j.
__device__ __forceinline__ uint4 read_fragment(const char* lds, int j, int h, int c) {
  return *reinterpret_cast<const uint4*>(lds + lds_chunk(j, h * 4 + c));
}

// acc += A-chunk x B-chunk: D[i][j] with i over a's tile rows and j over b's.
template <typename T>
__device__ __forceinline__ void mma_chunk(f32x16& acc, const uint4& a, const uint4& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (std::is_same<T, float>::value) {
    const f32x4 av = __builtin_bit_cast(f32x4, a), bv = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
  } else if constexpr (std::is_same<T, bf16>::value) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                  __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                 __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  }
#else
  (void)acc, (void)a, (void)b;
#endif
}

__host__ __device__ __forceinline__ bool aligned16(const void* p, int64_t ld_bytes) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld_bytes & 15) == 0;
}

}  // namespace segmm
}  // namespace ofx

#endif  // OFX_SEGMENT_MATMUL_DEV_H_
