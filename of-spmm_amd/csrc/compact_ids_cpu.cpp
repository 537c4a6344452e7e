// compact_ids_cpu.cpp — the kCPU kernel of the block compaction: the same arrays as
// compact_ids.hip (layout rules in compact_ids.h, contract in include/ofx_spmm.h).
// The same passes over the same bitmap: mark (atomic fetch-or), tile counts, a serial scan of the
// tile counts, emit (ranks and src, tile by tile), relabel.  Every pass but the scan runs under
// OpenMP; what each writes is fixed by the set of ids alone, so the output does not depend on
// num_threads.
#include <omp.h>

#include <vector>

#include "compact_ids.h"
#include "ofx_internal.h"
#include "spmm_common.h"

using namespace ofx;

namespace {

template <typename I>
int64_t id_at(const I* seeds, int64_t n_seeds, const I* cols, int64_t i) {
  return i < n_seeds ? (int64_t)seeds[i] : (int64_t)cols[i - n_seeds];
}

// Sets the bit of every good id; the position of the first bad one among the S + E ids, or -1.
template <typename I>
int64_t cpu_mark(int nthreads, int64_t num_nodes, int64_t n_seeds, const I* seeds, const I* cols,
                 int64_t n, uint32_t* bitmap) {
  int64_t first_bad = INT64_MAX;
#pragma omp parallel for num_threads(nthreads) schedule(static) reduction(min : first_bad)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = id_at(seeds, n_seeds, cols, i);
    if (!cid::id_ok(v, num_nodes)) {
      if (i < first_bad) first_bad = i;
      continue;
    }
    uint32_t* word = bitmap + (v >> 5);
    const uint32_t bit = 1u << (unsigned)(v & 31);
    if ((__atomic_load_n(word, __ATOMIC_RELAXED) & bit) == 0u)
      __atomic_fetch_or(word, bit, __ATOMIC_RELAXED);
  }
  return first_bad == INT64_MAX ? -1 : first_bad;
}

void cpu_tile_counts(int nthreads, int64_t tiles, const uint32_t* bitmap, int32_t* tile_count) {
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t t = 0; t < tiles; ++t) {
    const uint32_t* w = bitmap + t * (cid::kTileBits / cid::kWordBits);
    int c = 0;
    for (int g = 0; g < cid::kTileGranules; ++g)
      c += cid::granule_count(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
    tile_count[t] = c;
  }
}

// tile_base[t]: the set bits in front of tile t.
template <typename I>
void cpu_emit(int nthreads, int64_t tiles, const uint32_t* bitmap, const int32_t* tile_base,
              int32_t* rank, I* src) {
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 4)
  for (int64_t t = 0; t < tiles; ++t) {
    int32_t r = tile_base[t];
    for (int64_t g = t * cid::kTileGranules; g < (t + 1) * cid::kTileGranules; ++g) {
      rank[g] = r;
      for (int k = 0; k < cid::kGranuleWords; ++k) {
        const int64_t base = g * cid::kGranuleBits + k * cid::kWordBits;
        for (uint32_t rest = bitmap[4 * g + k]; rest != 0u; rest &= rest - 1u)
          src[r++] = (I)(base + __builtin_ctz(rest));
      }
    }
  }
}

template <typename I>
void cpu_relabel(int nthreads, int64_t n_seeds, const I* seeds, const I* cols, int64_t n,
                 const uint32_t* bitmap, const int32_t* rank, int64_t* seed_pos, I* col_local) {
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = id_at(seeds, n_seeds, cols, i);
    const int64_t g = v >> 7;
    const uint32_t* w = bitmap + 4 * g;
    const int pos = rank[g] + cid::granule_below(w[0], w[1], w[2], w[3], (int)(v & 127));
    if (i < n_seeds)
      seed_pos[i] = (int64_t)pos;
    else
      col_local[i - n_seeds] = (I)pos;
  }
}

}  // namespace

extern "C" int ofx_compact_ids_cpu(int num_threads, int idx_dtype, int64_t num_nodes,
                                   int64_t n_seeds, const void* seeds, int64_t n_cols,
                                   const void* cols, void* out_src, void* out_seed_pos,
                                   void* out_col_local, int64_t* out_count) {
  return ::ofx::guarded(__func__, [&]() -> int {
    const int rc = cid::check_compact_args("compact_ids_cpu", idx_dtype, num_nodes, n_seeds, seeds,
                                           n_cols, cols, out_src, out_seed_pos, out_col_local,
                                           out_count);
    if (rc) return rc;
    const int nt = threads_of(num_threads);
    *out_count = 0;
    const int64_t n = n_seeds + n_cols;
    if (n == 0) return OFX_OK;
    return by_index(idx_dtype, [&](auto* ip) -> int {
      using I = std::remove_pointer_t<decltype(ip)>;
      const int64_t tiles = cid::tiles_of(num_nodes);
      std::vector<uint32_t> bitmap((size_t)tiles * (cid::kTileBits / cid::kWordBits));  // cleared
      const int64_t bad = cpu_mark<I>(nt, num_nodes, n_seeds, (const I*)seeds, (const I*)cols, n,
                                      bitmap.data());
      OFX_REQUIRE(bad < 0, OFX_EINVAL,
                  "compact_ids_cpu: id %lld at position %lld of the seeds and columns is outside "
                  "[0, %lld)",
                  (long long)id_at((const I*)seeds, n_seeds, (const I*)cols, bad), (long long)bad,
                  (long long)num_nodes);
      std::vector<int32_t> tile((size_t)tiles + 1), rank((size_t)tiles * cid::kTileGranules);
      cpu_tile_counts(nt, tiles, bitmap.data(), tile.data() + 1);
      for (int64_t t = 0; t < tiles; ++t) tile[t + 1] += tile[t];  // tile[t]: the base of tile t
      cpu_emit<I>(nt, tiles, bitmap.data(), tile.data(), rank.data(), (I*)out_src);
      cpu_relabel<I>(nt, n_seeds, (const I*)seeds, (const I*)cols, n, bitmap.data(), rank.data(),
                     (int64_t*)out_seed_pos, (I*)out_col_local);
      *out_count = (int64_t)tile[tiles];
      return OFX_OK;
    });
  });
}
