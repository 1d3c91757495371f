// region_kernels.hpp -- coherent regions (gb25_label_regions, gb25_get_regions: include/gb25.h): connected-component labelling of
// a thresholded plane of a centre-located quantity, level by level, and one record per region whose sums run in a fixed order.
// Included by gb25_api.hip, launched from region_host.hpp, eight launches per level on the model's stream.  n = Nx Ny cells of
// one level, linear index c = i + Nx j; every kernel but the scan and the records takes one cell per thread, 256 per block (four
// waves of 64 consecutive indices).
//
//   k_region_init     the foreground of include/gb25.h -- x < threshold (or >) in `real`, x finite, mu > 0 with mu THE MEASURE of
//                     gb25_integrate_field (measure_column, measure_level of diagnostics_kernels.hpp) -- and the first forest:
//                     work[c] = -1 in the background, in the foreground the head of the cell's horizontal run inside its wave (two
//                     ballots, no memory is read for it).  Every link, here and below, goes to a SMALLER OR EQUAL index of the
//                     same region, so a tree's root is where work[c] == c and the one root a region ends with is its smallest
//                     index: the key.  The foreground and the non-finite wet cells are counted: lane 0 adds the wave's popcounts
//                     to the level's counts (integer atomics).
//   k_region_flatten  work[c] = the root above c: a walk of at most n hops (region_find).  Others shorten links meanwhile, always
//                     to an ancestor: the walk ends at a root whatever it reads.  With COUNT the block's roots are counted
//                     (roots are final once the merge has run).
//   k_region_merge    label equivalence: a cell whose western or southern neighbour is foreground, and a cell of column 0 whose
//                     neighbour across the seam (column Nx - 1, periodic grids) is, joins the two trees where they differ:
//                     atomicMin on the larger ROOT with the smaller; where the larger was no root any more the round goes on
//                     with what stood there (region_union).
//   k_region_scan     ONE block: the exclusive scan of the blocks' root counts, 256 at a time with a running carry; the total is the
//                     level's number of regions.
//   k_region_number   a root's number = its block's offset + the roots below it in the block (ballots and popcounts): ascending
//                     key order by construction.  num[key] = the number; the roots numbered below max_regions start their record
//                     (the key, j_min = the key's row: the smallest index lies in the lowest row).
//   k_region_rewrite  labels[c] = num[work[c]], -1 in the background; the box of a stored region by integer atomicMin / atomicMax
//                     from the cells ON its rim alone (no same-region neighbour on that side), `wraps` from column 0.
//   k_region_records  ONE WAVE per stored region marches the rows j_min .. j_max, the columns i_min .. i_max 64 at a time: the lanes
//                     load and form the terms (coalesced, in parallel), through LDS every lane then adds them ONE BY ONE in ascending
//                     linear index -- acc = acc + term, fp64, contraction off --, so the order of every sum is a function of the
//                     region alone.  Cost: the box's area.
//
// Every loop has a static bound: a walk n hops, a union Nx + Ny rounds of two walks each -- at most 2 n (Nx + Ny) loads per
// union, a bound that is formal: after the first flatten a walk is a hop or two -- (each raises `gave_up` in the level's counts when
// it runs out: the host reports it), the scan ceil(blocks / 256) chunks, the march Ny rows x ceil(Nx / 64) chunks x 64 terms.  No block waits for
// another: no flag is spun on, no look-back, no grid sync; the order of the launches on the stream is the only order.  Integer
// atomics on vector memory only, no floating-point atomics; nothing here writes model memory.
#pragma once
#include "diagnostics_kernels.hpp"

namespace gb25 {

constexpr int REG_THREADS = 256;   // cells of a block: four waves

struct RegionRecord {   // = gb25_region
  int cells, key_i, key_j, i_min, i_max, j_min, j_max, wraps, extreme_i, extreme_j;
  double measure, first, second, carried, sum_di, sum_dj, extreme;
};
struct RegionCounts {   // of one level
  int regions, foreground, nonfinite, gave_up;
};
struct RegionArgs {
  int Nx, Ny, n;             // n = Nx Ny
  int k;                     // the level in the field
  int above;                 // 0: x < threshold, 1: x >
  int periodic;              // column Nx - 1 is the neighbour of column 0
  int max_regions;
  real threshold;
  int* work;                 // n: the forest, then the keys
  int* num;                  // n: at a key, the number of its region
  int* block_roots;          // ceil(n / 256): the blocks' root counts, then their exclusive scan
  int* labels;               // n: the level's label plane
  RegionRecord* records;     // max_regions: the level's records
  RegionCounts* counts;      // the level's
};

__device__ __forceinline__ int region_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above c; at most n hops (the forest has no cycle: every link goes down)
__device__ __forceinline__ int region_find(const int* work, int c, int n, RegionCounts* counts) {
  int r = c;
  for (int hop = 0; hop < n; hop++) {
    const int p = region_load(work + r);
    if (p == r) return r;
    r = p;
  }
  atomicMax(&counts->gave_up, 1);
  return r;
}
// join the trees of a and b; `rounds` = Nx + Ny.  A round fails only when another thread has hung the larger root elsewhere between
// this thread's walk and its atomicMin, and then the thread's node strictly decreases: a handful of rounds in practice, so a bound
// far below n never ends a correct union, and one that it does end is worth reporting.
__device__ __forceinline__ void region_union(int* work, int a, int b, int n, int rounds, RegionCounts* counts) {
  for (int round = 0; round < rounds; round++) {
    a = region_find(work, a, n, counts);
    b = region_find(work, b, n, counts);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(work + a, b);   // a > b
    if (old == a) return;                     // a was a root: it hangs below b now
    a = old;                                  // it was not: what it hung below joins b (or b it)
  }
  atomicMax(&counts->gave_up, 1);
}

// x: the criterion, box.origin its element (0, 0, first level of the window); K: the level in the window
template <class T>
__global__ __launch_bounds__(REG_THREADS) void k_region_init(Grid g, MomentsTables tab, const T* __restrict__ x, DiagBox box, int K, RegionArgs A) {
  const int c = blockIdx.x * REG_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const bool inside = c < A.n;
  const int j = inside ? c / A.Nx : 0, i = inside ? c - j * A.Nx : 0;
  bool fg = false, bad = false;
  if (inside) {
    const MeasureColumn mc = measure_column<0>(g, tab, i, j);
    if (measure_level<LOC_CCC>(g, mc, A.k) > 0.0) {
      const T v = x[box.origin + box.pitch * j + box.plane * K + i];
      bad = !__builtin_isfinite(v);
      fg = !bad && (A.above ? v > A.threshold : v < A.threshold);
    }
  }
  // (whole waves: nobody has returned)
  const unsigned long long fgm = __ballot(fg), row0 = __ballot(inside && i == 0), badm = __ballot(bad);
  if (fg) {
    // the heads of the runs inside the wave: a foreground lane whose western lane is none, or lies in the row below
    const unsigned long long heads = fgm & ~((fgm << 1) & ~row0);
    const unsigned long long upto = heads & ((2ull << lane) - 1ull);   // (not empty: a foreground lane has a head at or below it)
    A.work[c] = c - (lane - (63 - __builtin_clzll(upto)));
  } else if (inside) {
    A.work[c] = -1;
  }
  if (lane == 0) {
    if (fgm) atomicAdd(&A.counts->foreground, __popcll(fgm));
    if (badm) atomicAdd(&A.counts->nonfinite, __popcll(badm));
  }
}

template <bool COUNT>
__global__ __launch_bounds__(REG_THREADS) void k_region_flatten(RegionArgs A) {
  __shared__ int wave_roots[REG_THREADS / 64];
  const int c = blockIdx.x * REG_THREADS + threadIdx.x;
  bool root = false;
  if (c < A.n && region_load(A.work + c) >= 0) {
    const int r = region_find(A.work, c, A.n, A.counts);
    if (r != c) A.work[c] = r;
    root = r == c;
  }
  if (COUNT) {
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0) wave_roots[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < REG_THREADS / 64; w++) s += wave_roots[w];
      A.block_roots[blockIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(REG_THREADS) void k_region_merge(RegionArgs A) {
  const int c = blockIdx.x * REG_THREADS + threadIdx.x;
  if (c >= A.n) return;
  const int mine = region_load(A.work + c);
  if (mine < 0) return;
  const int j = c / A.Nx, i = c - j * A.Nx;
  int other[3];
  other[0] = i > 0 ? c - 1 : -1;
  other[1] = j > 0 ? c - A.Nx : -1;
  other[2] = (A.periodic && i == 0 && A.Nx > 1) ? c + A.Nx - 1 : -1;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (other[q] < 0) continue;
    const int theirs = region_load(A.work + other[q]);
    if (theirs < 0 || theirs == region_load(A.work + c)) continue;
    region_union(A.work, c, other[q], A.n, A.Nx + A.Ny, A.counts);
  }
}

// one block; blocks: how many counts there are
__global__ __launch_bounds__(REG_THREADS) void k_region_scan(RegionArgs A, int blocks) {
  __shared__ int s[REG_THREADS];
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < blocks; base += REG_THREADS) {
    const int at = base + t;
    const int v = at < blocks ? A.block_roots[at] : 0;
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < REG_THREADS; off <<= 1) {
      const int below = t >= off ? s[t - off] : 0;
      __syncthreads();
      s[t] += below;
      __syncthreads();
    }
    if (at < blocks) A.block_roots[at] = carry + s[t] - v;
    carry += s[REG_THREADS - 1];
    __syncthreads();
  }
  if (t == 0) A.counts->regions = carry;
}

__global__ __launch_bounds__(REG_THREADS) void k_region_number(RegionArgs A) {
  __shared__ int wave_roots[REG_THREADS / 64];
  const int c = blockIdx.x * REG_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool root = c < A.n && A.work[c] == c;
  const unsigned long long m = __ballot(root);
  if (lane == 0) wave_roots[wave] = __popcll(m);
  __syncthreads();
  if (!root) return;
  int r = A.block_roots[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; w++) r += wave_roots[w];
  A.num[c] = r;
  if (r < A.max_regions) {
    RegionRecord rec = {};
    rec.key_j = c / A.Nx;
    rec.key_i = c - rec.key_j * A.Nx;
    rec.i_min = rec.i_max = rec.key_i;
    rec.j_min = rec.j_max = rec.key_j;
    A.records[r] = rec;
  }
}

__global__ __launch_bounds__(REG_THREADS) void k_region_rewrite(RegionArgs A) {
  const int c = blockIdx.x * REG_THREADS + threadIdx.x;
  if (c >= A.n) return;
  const int key = A.work[c];
  if (key < 0) {
    A.labels[c] = -1;
    return;
  }
  const int r = A.num[key];
  A.labels[c] = r;
  if (r >= A.max_regions) return;
  RegionRecord* rec = A.records + r;
  const int j = c / A.Nx, i = c - j * A.Nx;
  if (!(i > 0 && A.work[c - 1] == key)) atomicMin(&rec->i_min, i);
  if (!(i < A.Nx - 1 && A.work[c + 1] == key)) atomicMax(&rec->i_max, i);
  if (!(j < A.Ny - 1 && A.work[c + A.Nx] == key)) atomicMax(&rec->j_max, j);
  if (A.periodic && i == 0 && A.Nx > 1 && A.work[c + A.Nx - 1] >= 0) atomicMax(&rec->wraps, 1);
}

// x, box, K as for k_region_init; y: the carried field's parent (null: none), ybox.origin its element (0, 0, A.k)
template <class T>
__global__ __launch_bounds__(64) void k_region_records(Grid g, MomentsTables tab, const T* __restrict__ x, DiagBox box, int K,
                                                       const T* __restrict__ y, DiagBox ybox, RegionArgs A) {
#pragma clang fp contract(off)
  __shared__ double term[7][64];   // mu, mu x, (mu x) x, mu y, mu di, mu dj, x
  const int r = blockIdx.x, lane = threadIdx.x;
  const int regions = A.counts->regions;
  if (r >= regions || r >= A.max_regions) return;   // (uniform for the block)
  RegionRecord rec = A.records[r];
  const int j0 = rec.j_min < 0 ? 0 : rec.j_min, j1 = rec.j_max > A.Ny - 1 ? A.Ny - 1 : rec.j_max;
  const int i0 = rec.i_min < 0 ? 0 : rec.i_min, i1 = rec.i_max > A.Nx - 1 ? A.Nx - 1 : rec.i_max;
  double measure = 0.0, first = 0.0, second = 0.0, carried = 0.0, sum_di = 0.0, sum_dj = 0.0;
  double extreme = A.above ? -__builtin_inf() : __builtin_inf();
  int extreme_at = -1, cells = 0;
  for (int j = j0; j <= j1; j++) {
    for (int base = i0; base <= i1; base += 64) {
      const int i = base + lane;
      const bool in = i <= i1 && A.labels[i + A.Nx * j] == r;
      if (in) {
        const MeasureColumn mc = measure_column<0>(g, tab, i, j);
        const double mu = measure_level<LOC_CCC>(g, mc, A.k);
        const double v = (double)x[box.origin + box.pitch * j + box.plane * K + i];
        int di = i - rec.key_i;
        if (A.periodic) di = 2 * di >= A.Nx ? di - A.Nx : (2 * di < -A.Nx ? di + A.Nx : di);
        const double t = mu * v;
        term[0][lane] = mu;
        term[1][lane] = t;
        term[2][lane] = t * v;
        term[3][lane] = y ? mu * (double)y[ybox.origin + ybox.pitch * j + i] : 0.0;
        term[4][lane] = mu * (double)di;
        term[5][lane] = mu * (double)(j - rec.key_j);
        term[6][lane] = v;
      }
      unsigned long long todo = __ballot(in);
      __syncthreads();
      for (int s = 0; s < 64 && todo; s++) {   // every lane adds every term: the same sums in every lane
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        measure = measure + term[0][l];
        first = first + term[1][l];
        second = second + term[2][l];
        carried = carried + term[3][l];
        sum_di = sum_di + term[4][l];
        sum_dj = sum_dj + term[5][l];
        const double v = term[6][l];
        if (A.above ? v > extreme : v < extreme) {
          extreme = v;
          extreme_at = base + l + A.Nx * j;
        }
        cells++;
      }
      __syncthreads();
    }
  }
  if (lane == 0) {
    rec.cells = cells;
    rec.measure = measure; rec.first = first; rec.second = second; rec.carried = carried;
    rec.sum_di = sum_di; rec.sum_dj = sum_dj;
    rec.extreme = cells ? extreme : 0.0;
    rec.extreme_j = cells ? extreme_at / A.Nx : 0;
    rec.extreme_i = cells ? extreme_at - rec.extreme_j * A.Nx : 0;
    A.records[r] = rec;
  }
}

}  // namespace gb25
