// Assignment of new points to the clusters of a finished train (pd_index_*).
//
//   predict(q) = min { label(c) : c core, dist(q, c) <= eps }     (-1: none)
//
// with the train's own predicate (pred.hpp) and the train's border rule (a
// border point takes the smallest key among its core neighbours, and labels
// rank the keys), so predict(X_train) == labels_ for core, border and noise
// points alike.
//
// The index owns its device memory (`keep`) and a private scratch context
// (`work`: sort buffers, compaction offsets, the pinned block), so no train on
// the caller's context can touch it.
//
// d <= 4 — a grid over the cores' tight bounding box, cells eps*(1 + 2^-20)
// wide on every axis (any pair the predicate accepts lies in adjacent cells):
//   Xs    T[nc * S]     core coordinates in cell order (S: Stride<D>)
//   lab   i32[nc]       their labels
//   ckey  K[ncells]     keys of the OCCUPIED cells, ascending (row-major, axis 0
//                       fastest)
//   cstart u32[ncells+1] first core of each occupied cell
//   clab  i32[ncells]   the label every core of the cell has, -1 when they differ
//   tab   u32[ntab]     lower bound in ckey of every key prefix (key >> shift)
// Memory follows the cores, never the extent: two blobs 1e6 apart cost what the
// blobs cost.  A query walks the 3^(d-1) rows around its cell; in each the
// (up to) three neighbour cells are one contiguous key run [k0, k1], found by
// one bucketed binary search over ckey, and their cores one contiguous record
// run.  Only a label below the best one so far can change the answer: a cell
// whose cores all share a label not below it is skipped whole, one that shares
// a smaller label is decided by its first hit, and in a mixed cell only the
// cores with a smaller label are tested (C2, the 1e8 training points: sweep
// kernel 34.8 -> 11.3 ms).  Cells grow by a common factor (exact at any width >= eps) only to keep
// every axis below 2^28 cells — the bound under which the fp64 rounding of the
// cell coordinate stays inside the 2^-20 margin — and the key below 2^62.
//
// d > 4 — the compacted core rows, swept as LDS tiles by every query
// (exact fp64, axis order; no MFMA screen: DESIGN.md §10).
//
// The same index built over ALL rows (mask of ones, eps = the cap r_max) also
// answers k-distance queries (pd_index_kdist): the k-th smallest
// accumulator within the cap, by the same row walk / tiles with a k-best list
// per lane in place of the minimum label — and radius queries
// (pd_index_radius_count / _fill): every row within a radius
// <= eps of each query, as CSR, by the same walk / tiles in a count pass, a
// 64-bit scan of the counts and a fill pass that writes each hit's label —
// and k-nearest queries (pd_index_kneighbors): the k-distance
// walk / tiles with a list of (accumulator, label) pairs, written out in order.
// Built with labels[i] = i it also yields the mutual-reachability forest
// (pd_index_mreach_forest; d <= 4): Borůvka rounds in which every
// record walks its rows for the lightest edge to a row of another component,
// behind a per-cell component short cut (ccomp, the analogue of clab);
// pd_forest_labels cuts such a forest into the train's labels.  Given the
// rows' sample_weight (pd_index_set_weights) the same index
// answers the weighted core accumulator (pd_index_kdist_weighted: the walk /
// tiles with a list of (accumulator, weight) pairs — WRegList, WLdsList — and
// the crossing of the running weight sum taken after it) and builds the forest
// on it (pd_index_mreach_forest_weighted).
//
// The four query kinds share one walk and one tile sweep; a
// kernel is a prologue, a sink, one call and its write-out.  The layers:
//   view      IxView: what a d <= 4 kernel reads of the index, by value
//             (view_of fills it from Index)
//   prologue  QueryAt: lane -> query (through `order`), its coordinates with
//             the finite check, its cell; a kernel decides what a non-finite
//             query or one outside the grid gets
//   rows      for_each_row: the 3^(D-1) rows around the cell, the query's own
//             first, each as the key run [klo, khi] of its <= 3 cells
//   run       first_cell / row_run: key run -> occupied cells -> the one record
//             run [j0, j1) that holds their rows
//   scan      scan_run: four records' loads and exact sums in flight, offered
//             to the sink in record order; walk = rows + run + scan
//   sinks     offer(acc, j) / tau(): RegList, LdsList (k best accumulators),
//             RegPairs, LdsPairs (k best (acc, label) pairs), RadiusRow (count
//             or fill), MinLabel (predict, d > 4)
//   tiles     d > 4: stage_queries (the block's queries transposed into LDS)
//             and tile_sweep (rows and labels streamed through LDS, the axis
//             loop that stops at the first partial sum above sink.tau())
// predict's d <= 4 kernel uses the prologue, the rows and first_cell and keeps
// its own per-cell loop (labels prune there, and Pred screens in fp32).
// kdist_kernel calls walk.  knn_kernel and radius_kernel have the walk written
// out after the shared prologue: through the helpers the first lost occupancy
// in eight instantiations and the second 0.7 - 1.5 % of its speed (DESIGN.md
// §15 has the figures).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "compact.hpp"
#include "internal.hpp"
#include "pred.hpp"
#include "uf.hpp"

namespace pd {

struct IxGrid {
    double lo[kMaxDim];       // origin: the cores' tight bbox
    double inv[kMaxDim];      // 1 / cell side
    int64_t nc[kMaxDim];      // cells per axis
    uint64_t stride[kMaxDim]; // key = sum c[j] * stride[j]
    uint64_t G;               // cells in all (also: the key of a query nothing can match)
};

struct Index {
    Ctx work;                 // scratch only
    Arena keep;               // what a query reads
    int device = 0, dtype = 0, d = 0, metric = 0;
    double eps = 0;
    uint64_t nc = 0;          // core points
    IxGrid g{};
    int key_bytes = 4, key_bits = 1, shift = 0;
    uint32_t ncells = 0;
    uint64_t ntab = 0;
    float slo = -1.0f, shi = INFINITY;
    void* Xs = nullptr;       // d <= 4: cell order, Stride<D>; d > 4: compacted rows
    int32_t* lab = nullptr;
    void* ckey = nullptr;
    uint32_t* cstart = nullptr;
    int32_t* clab = nullptr;
    uint32_t* tab = nullptr;
    // pd_index_set_weights: the rows' fixed-point weights in the
    // index's own order, clamped to kWeightClamp; wmin: the smallest non-zero
    // unclamped one (0: no row has weight)
    uint64_t n_rows = 0;      // rows given to the build
    uint32_t* wrec = nullptr;
    uint64_t wmin = 0;
    bool weighted = false;
};

namespace {

// Queries per call from which they are swept in cell order (key, sort, sweep
// through the order) instead of input order: measured on C2 (tools/
// predict_bench.py, ms sorted / direct) 65536: 0.16 / 0.10, 262144: 0.22 /
// 0.21, 1e6: 0.43 / 0.99, 1e8: 14.1 / 178.  PD_INDEX_SORT_MIN overrides it per
// call (that A/B, and the tests; same results either way).
constexpr uint64_t kSortMin = 1 << 18;
uint64_t sort_min() {
    const char* e = std::getenv("PD_INDEX_SORT_MIN");
    if (!e || !*e) return kSortMin;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    return end && *end == 0 ? (uint64_t)v : kSortMin;
}
constexpr int64_t kMaxAxisCells = 1ll << 28;
constexpr int kStatSlots = 2 + 2 * kMaxDim;  // non-finite, negative labels, min[4], max[4]

struct CorePred {
    const uint8_t* core;
    __device__ bool operator()(uint32_t i) const { return core[i] != 0; }
};

template <typename K>
struct HeadPred {
    const K* keys;
    __device__ bool operator()(uint32_t i) const { return i == 0 || keys[i] != keys[i - 1]; }
};

// order-preserving u64 image of a double (for atomicMin / atomicMax)
__device__ __forceinline__ unsigned long long enc_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double dec_f64(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    double v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

// Non-finite coordinates and negative labels among the core rows; for
// d <= kMaxDim also their tight bbox.  stats: see kStatSlots (min slots start
// at ~0, max slots at 0).
template <typename T>
__global__ __launch_bounds__(kBlock) void core_stats_kernel(const T* __restrict__ X, int d,
                                                            const uint32_t* __restrict__ clist,
                                                            uint64_t nc,
                                                            const int32_t* __restrict__ labels,
                                                            unsigned long long* __restrict__ stats) {
    const bool box = d <= kMaxDim;
    double mn[kMaxDim], mx[kMaxDim];
#pragma unroll
    for (int j = 0; j < kMaxDim; ++j) {
        mn[j] = INFINITY;
        mx[j] = -INFINITY;
    }
    unsigned bad = 0, neg = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nc;
         i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t p = clist[i];
        neg += labels[p] < 0 ? 1u : 0u;
        if (box) {
#pragma unroll
            for (int j = 0; j < kMaxDim; ++j) {
                if (j < d) {
                    const double v = (double)X[p * d + j];
                    if (!isfinite(v)) {
                        ++bad;
                    } else {
                        mn[j] = fmin(mn[j], v);
                        mx[j] = fmax(mx[j], v);
                    }
                }
            }
        } else {
            for (int j = 0; j < d; ++j) bad += isfinite((double)X[p * d + j]) ? 0u : 1u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += (unsigned)__shfl_xor((int)bad, o, 64);
        neg += (unsigned)__shfl_xor((int)neg, o, 64);
#pragma unroll
        for (int j = 0; j < kMaxDim; ++j) {
            mn[j] = fmin(mn[j], __shfl_xor(mn[j], o, 64));
            mx[j] = fmax(mx[j], __shfl_xor(mx[j], o, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(stats + 0, (unsigned long long)bad);
        if (neg) atomicAdd(stats + 1, (unsigned long long)neg);
        if (box) {
            for (int j = 0; j < d; ++j) {
                if (mn[j] <= mx[j]) {
                    atomicMin(stats + 2 + j, enc_f64(mn[j]));
                    atomicMax(stats + 2 + kMaxDim + j, enc_f64(mx[j]));
                }
            }
        }
    }
}

// Cell coordinate of v along every axis, in the arithmetic the host sized the
// grid with: floor((v - lo) * inv), each operation rounded on its own.
// Returns false when v lies more than one cell outside the grid (nothing can
// be within eps of it); otherwise c[j] is in [-1, nc[j]].
template <int D>
__device__ __forceinline__ bool cell_of(const double (&v)[D], const IxGrid& g, int64_t (&c)[D]) {
    bool in = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const double s = __dmul_rn(__dadd_rn(v[j], -g.lo[j]), g.inv[j]);
        const bool ok = (s >= -1.0) && (s < (double)g.nc[j] + 1.0);
        in = in && ok;
        c[j] = ok ? (int64_t)floor(s) : 0;
    }
    return in;
}

template <int D>
__device__ __forceinline__ uint64_t clamped_key(const int64_t (&c)[D], const IxGrid& g) {
    uint64_t k = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        int64_t q = c[j] < 0 ? 0 : c[j];
        q = q >= g.nc[j] ? g.nc[j] - 1 : q;
        k += (uint64_t)q * g.stride[j];
    }
    return k;
}

template <typename T, int D, typename K>
__global__ __launch_bounds__(kBlock) void core_key_kernel(const T* __restrict__ X,
                                                          const uint32_t* __restrict__ clist,
                                                          uint64_t nc, IxGrid g,
                                                          K* __restrict__ keys,
                                                          uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nc) return;
    const uint64_t p = clist[i];
    double v[D];
#pragma unroll
    for (int j = 0; j < D; ++j) v[j] = (double)X[p * D + j];
    int64_t c[D];
    (void)cell_of<D>(v, g, c);   // a core is inside the box: always in
    keys[i] = (K)clamped_key<D>(c, g);
    vals[i] = (uint32_t)i;
}

// Coordinates (Stride<D> layout, pad 0) and labels into cell order.
template <typename T, int D>
__global__ __launch_bounds__(kBlock) void core_gather_kernel(const T* __restrict__ X,
                                                             const uint32_t* __restrict__ clist,
                                                             const uint32_t* __restrict__ vals,
                                                             const int32_t* __restrict__ labels,
                                                             uint64_t nc, T* __restrict__ Xs,
                                                             int32_t* __restrict__ lab) {
    constexpr int S = Stride<D>::v;
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= nc) return;
    const uint64_t p = clist[vals[r]];
#pragma unroll
    for (int j = 0; j < S; ++j) Xs[r * S + j] = j < D ? X[p * D + j] : (T)0;
    lab[r] = labels[p];
}

// d > kMaxDim: the compacted rows as they are.
template <typename T>
__global__ __launch_bounds__(kBlock) void rows_gather_kernel(const T* __restrict__ X, int d,
                                                             const uint32_t* __restrict__ clist,
                                                             const int32_t* __restrict__ labels,
                                                             uint64_t nc, T* __restrict__ Xc,
                                                             int32_t* __restrict__ lab) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= nc * (uint64_t)d) return;
    const uint64_t r = e / (uint64_t)d, k = e % (uint64_t)d;
    const uint64_t p = clist[r];
    Xc[e] = X[p * d + k];
    if (k == 0) lab[r] = labels[p];
}

// ckey[c] = key of occupied cell c; cstart gets its end sentinel.
template <typename K>
__global__ __launch_bounds__(kBlock) void cell_keys_kernel(const K* __restrict__ keys,
                                                           uint32_t* __restrict__ cstart,
                                                           uint32_t ncells, uint32_t nc,
                                                           K* __restrict__ ckey) {
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c < ncells) ckey[c] = keys[cstart[c]];
    if (c == ncells) cstart[c] = nc;
}

// clab[c] = the label all cores of cell c share, -1 when they differ.
__global__ __launch_bounds__(kBlock) void cell_label_kernel(const uint32_t* __restrict__ cstart,
                                                            const int32_t* __restrict__ lab,
                                                            uint32_t ncells,
                                                            int32_t* __restrict__ clab) {
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncells) return;
    const uint32_t j1 = cstart[c + 1];
    uint32_t j = cstart[c];
    const int32_t l = lab[j];
    for (++j; j < j1 && lab[j] == l; ++j) {}
    clab[c] = j == j1 ? l : -1;
}

template <typename K>
__device__ __forceinline__ uint32_t cell_lower_bound(const K* __restrict__ ckey, uint32_t lo,
                                                uint32_t hi, uint64_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)ckey[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// tab[b] = first occupied cell whose key is >= b << shift.
template <typename K>
__global__ __launch_bounds__(kBlock) void cell_tab_kernel(const K* __restrict__ ckey,
                                                          uint32_t ncells, int shift,
                                                          uint64_t ntab,
                                                          uint32_t* __restrict__ tab) {
    const uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= ntab) return;
    tab[b] = cell_lower_bound<K>(ckey, 0u, ncells, b << shift);
}

// Key of each query's own (clamped) cell; G for a query nothing can match.
template <typename T, int D, typename K>
__global__ __launch_bounds__(kBlock) void query_key_kernel(const T* __restrict__ Q, uint64_t m,
                                                           IxGrid g, K* __restrict__ keys,
                                                           uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    double v[D];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        v[j] = (double)Q[i * D + j];
        fin = fin && isfinite(v[j]);
    }
    int64_t c[D];
    const bool in = fin && cell_of<D>(v, g, c);
    keys[i] = in ? (K)clamped_key<D>(c, g) : (K)g.G;
    vals[i] = (uint32_t)i;
}

template <int D>
struct Rows {
    static constexpr int v = D == 1 ? 1 : D == 2 ? 3 : D == 3 ? 9 : 27;
};

// Device-side bounds checks of the query kernels, engine.hip's scheme
// (-DPD_CHECK_BOUNDS=1 builds): a checked access that would leave its buffer
// is skipped and the first one recorded; the host reads the record after the
// kernel and throws.  Off (the default) PD_OK is `true` and costs nothing.
// Sites: 40 a query number from `order`; 41 the key prefix into `tab`; 42 a
// row's record run (covers Xs and lab alike); 43 / 44 a tile's rows / labels;
// 45 a query's pair of radius offsets; 46 a k-nearest output slot; the forest
// (DESIGN.md §16): 47 a record-order read (cd_rec, comp_rec, the bests); 48 a
// component table (comp, par, best_w, best_uv: row numbers); 49 the edge append.
#ifndef PD_CHECK_BOUNDS
#define PD_CHECK_BOUNDS 0
#endif
#if PD_CHECK_BOUNDS
__device__ unsigned long long g_ix_oob[2];   // [0] violations, [1] the first
__device__ __forceinline__ bool pd_ix_ok(bool c, unsigned site, uint64_t idx) {
    if (!c && atomicAdd(&g_ix_oob[0], 1ull) == 0ull)
        g_ix_oob[1] = ((unsigned long long)site << 48) | (idx & 0xFFFFFFFFFFFFull);
    return c;
}
#define PD_OK(cond, site, idx) pd_ix_ok((cond), (site), (uint64_t)(idx))
#else
#define PD_OK(cond, site, idx) true
#endif

// ------------------------------------------------------------ the shared walk
// What a d <= 4 query kernel reads of the index (view_of fills it).
template <typename T, typename K>
struct IxView {
    IxGrid g;
    const T* Xs;
    const int32_t* lab;
    uint64_t nrec;   // rows of Xs, entries of lab
    const K* ckey;
    const uint32_t* cstart;
    const int32_t* clab;
    const uint32_t* tab;
    uint64_t ntab;
    uint32_t ncells;
    int shift;
};

enum Where : int {
    kPast,        // no query: a lane past m
    kNonFinite,   // a NaN or infinite coordinate (tallied in `bad`)
    kOutside,     // more than a cell outside the grid: nothing can be within eps
    kInGrid
};

// The prologue of a lane (block of `lanes`): its query — order[i] when the
// queries are swept in cell order (`order` nullable), results go to row qi of
// the outputs —, the coordinates as stored and widened, and the cell.
template <typename T, int D>
struct QueryAt {
    uint64_t qi;
    T ar[D];
    double a[D];
    int64_t c[D];   // kInGrid only
    Where where;
    __device__ __forceinline__ QueryAt(const T* __restrict__ Q, uint64_t m,
                                       const uint32_t* __restrict__ order, const IxGrid& g,
                                       unsigned long long* __restrict__ bad, unsigned lanes) {
        const uint64_t i = (uint64_t)blockIdx.x * lanes + threadIdx.x;
        qi = 0;
        where = kPast;
        if (i >= m) return;
        qi = order ? (uint64_t)order[i] : i;
        if (!PD_OK(qi < m, 40, qi)) return;
        bool fin = true;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            ar[j] = Q[qi * D + j];
            a[j] = (double)ar[j];
            fin = fin && isfinite(a[j]);
        }
        if (!fin) {
            atomicAdd(bad, 1ull);
            where = kNonFinite;
            return;
        }
        where = cell_of<D>(a, g, c) ? kInGrid : kOutside;
    }
};

// The 3^(D-1) rows of cells around cell c that lie inside the grid, the cell's
// own row first (its candidates usually settle the rest: predict's first hit,
// a list's small values): f(klo, khi), the keys of the row's first and last
// cell (axis 0: c[0] - 1 .. c[0] + 1, clamped).
template <int D, typename F>
__device__ __forceinline__ void for_each_row(const IxGrid& g, const int64_t (&c)[D], F&& f) {
    const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
    const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
    for (int rq = 0; rq < Rows<D>::v; ++rq) {
        const int r = (rq + Rows<D>::v / 2) % Rows<D>::v;
        uint64_t base = 0;
        bool ok = true;
        int rr = r;
#pragma unroll
        for (int ax = D - 1; ax >= 1; --ax) {
            // r in base 3, axis D-1 the most significant digit
            int pw = 1;
            for (int t = 1; t < ax; ++t) pw *= 3;
            const int64_t y = c[ax] + (int64_t)(rr / pw) - 1;
            rr %= pw;
            ok = ok && y >= 0 && y < g.nc[ax];
            base += (uint64_t)(ok ? y : 0) * g.stride[ax];
        }
        if (!ok) continue;
        f(base + (uint64_t)x0, base + (uint64_t)x1);
    }
}

// The first occupied cell with a key >= klo: one bucketed binary search.
template <typename T, typename K>
__device__ __forceinline__ uint32_t first_cell(const IxView<T, K> v, uint64_t klo) {
    const uint64_t b = klo >> v.shift;
    if (!PD_OK(b + 1 < v.ntab, 41, b)) return v.ncells;
    return cell_lower_bound<K>(v.ckey, v.tab[b], v.tab[b + 1], klo);
}

// Occupied cells adjacent in ckey hold adjacent records, so the cells of a row
// are one record run [j0, j1).  False when the row has no occupied cell.
template <typename T, typename K>
__device__ __forceinline__ bool row_run(const IxView<T, K> v, uint64_t klo, uint64_t khi,
                                        uint32_t& j0, uint32_t& j1) {
    const uint32_t e0 = first_cell(v, klo);
    uint32_t e1 = e0;
    for (; e1 < v.ncells && (uint64_t)v.ckey[e1] <= khi; ++e1) {}   // <= 3 cells
    if (e1 == e0) return false;
    j0 = v.cstart[e0];
    j1 = v.cstart[e1];
    return PD_OK(j0 <= j1 && j1 <= v.nrec, 42, j1);
}

template <typename T, int D, int M>
__device__ __forceinline__ double rec_acc(const T* __restrict__ Xs, uint32_t j,
                                          const double (&a)[D]) {
    double bv[D];
    load_rec<T, D>(Xs, j, bv);
    double acc = 0.0;
#pragma unroll
    for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
    return acc;
}

// Every record of [j, j1) to the sink, in record order.  Four candidates' loads
// and sums are issued together (the loads do not wait on the sink).
template <typename T, int D, int M, typename S>
__device__ __forceinline__ void scan_run(const T* __restrict__ Xs, const double (&a)[D], uint32_t j,
                                         uint32_t j1, S& sink) {
    for (; j + 4 <= j1; j += 4) {
        double acc4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc4[u] = rec_acc<T, D, M>(Xs, j + u, a);
#pragma unroll
        for (int u = 0; u < 4; ++u) sink.offer(acc4[u], j + u);
    }
    for (; j < j1; ++j) sink.offer(rec_acc<T, D, M>(Xs, j, a), j);
}

// Every candidate of an in-grid query, with its exact fp64 accumulator, to the
// sink: sink.offer(acc, j), j the record (lab[j] its label).
template <typename T, int D, int M, typename K, typename S>
__device__ __forceinline__ void walk(const IxView<T, K> v, const QueryAt<T, D> q, S& sink) {
    for_each_row<D>(v.g, q.c, [&](uint64_t klo, uint64_t khi) {
        uint32_t j0, j1;
        if (row_run(v, klo, khi, j0, j1)) scan_run<T, D, M>(v.Xs, q.a, j0, j1, sink);
    });
}

// predict, d <= 4.  One lane per query; in each row the cells of the key run;
// fp32 screen + exact fp64 recheck (Pred) of the cores whose label could lower
// the answer; the smallest label among the hits.
template <typename T, int D, int M, typename K>
__global__ __launch_bounds__(kBlock) void query_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    double eps, double eps2, float slo, float shi, int32_t* __restrict__ out,
    unsigned long long* __restrict__ bad) {
    const QueryAt<T, D> q(Q, m, order, v.g, bad, kBlock);
    if (q.where == kPast) return;
    if (q.where != kInGrid) {
        out[q.qi] = -1;
        return;
    }
    Pred<T, D, M> pr;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        pr.ar[j] = q.ar[j];
        pr.a[j] = q.a[j];
    }
    pr.eps = eps;
    pr.eps2 = eps2;
    pr.lo = slo;
    pr.hi = shi;
    int32_t best = INT32_MAX;
    for_each_row<D>(v.g, q.c, [&](uint64_t klo, uint64_t khi) {
        for (uint32_t e = first_cell(v, klo); e < v.ncells && (uint64_t)v.ckey[e] <= khi; ++e) {
            const int32_t cl = v.clab[e];
            const uint32_t j1 = v.cstart[e + 1];
            uint32_t j = v.cstart[e];
            if (cl >= 0) {
                if (cl >= best) continue;
                for (; j < j1; ++j) {
                    T bv[D];
                    load_raw<T, D>(v.Xs, j, bv);
                    if (pr(bv)) {
                        best = cl;
                        break;
                    }
                }
            } else {
                for (; j < j1; ++j) {
                    const int32_t l = v.lab[j];
                    if (l >= best) continue;
                    T bv[D];
                    load_raw<T, D>(v.Xs, j, bv);
                    if (pr(bv)) best = l;
                }
            }
        }
    });
    out[q.qi] = best == INT32_MAX ? -1 : best;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void finite_kernel(const T* __restrict__ Q, uint64_t total,
                                                        unsigned long long* __restrict__ bad) {
    unsigned c = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * kBlock)
        c += isfinite((double)Q[e]) ? 0u : 1u;
    if (c) atomicAdd(bad, (unsigned long long)c);
}

// ------------------------------------------------------------- the tile sweep
// d > kMaxDim.  A block of QB lanes owns QB queries, kept transposed in LDS
// (Qs[k][lane]: conflict-free); the rows pass through LDS in tiles of TC
// (every lane reads the same row element: a broadcast).  Each pair runs the
// predicate's own fp64 sum in axis order (within_axis) and stops at the first
// partial sum above the sink's bound — the sum never decreases, so the outcome
// is that of the full sum, and a pair that is offered ran to the end: its
// accumulator is the full sum.

// The block's queries into Qs[k][lane] (zero rows past m), non-finite
// coordinates tallied in `bad`.
template <typename T>
__device__ __forceinline__ void stage_queries(const T* __restrict__ Q, uint64_t m, int d, T* Qs,
                                              unsigned long long* __restrict__ bad) {
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    const uint64_t q0 = (uint64_t)blockIdx.x * QB;
    unsigned nf = 0;
    for (int e = tid; e < QB * d; e += QB) {
        const int row = e / d, k = e % d;
        const uint64_t gi = q0 + (uint64_t)row;
        const T v = gi < m ? Q[gi * (uint64_t)d + k] : (T)0;
        nf += isfinite((double)v) ? 0u : 1u;
        Qs[(size_t)k * QB + row] = v;
    }
    if (nf) atomicAdd(bad, (unsigned long long)nf);
}

// Every row of Xc against this lane's staged query: Cs[TC][d] holds the tile,
// Ls[TC] its labels when the sink reads them (LABELS; it is then given Ls, and
// j is the row's place in the tile).  A lane that is not `live` keeps the
// barriers and sweeps nothing.
template <typename T, int M, bool LABELS, typename S>
__device__ __forceinline__ void tile_sweep(const T* __restrict__ Xc,
                                           const int32_t* __restrict__ lab, uint64_t nc, int d,
                                           int TC, const T* Qs, T* Cs, int32_t* Ls, bool live,
                                           S& sink) {
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    for (uint64_t t0 = 0; t0 < nc; t0 += (uint64_t)TC) {
        const int tc = (int)(nc - t0 < (uint64_t)TC ? nc - t0 : (uint64_t)TC);
        __syncthreads();
        for (int e = tid; e < tc * d; e += QB)
            if (PD_OK(t0 * (uint64_t)d + e < nc * (uint64_t)d, 43, t0 * (uint64_t)d + e))
                Cs[e] = Xc[t0 * (uint64_t)d + e];
        if constexpr (LABELS)
            for (int e = tid; e < tc; e += QB)
                if (PD_OK(t0 + e < nc, 44, t0 + e)) Ls[e] = lab[t0 + e];
        __syncthreads();
        if (!live) continue;
        for (int c = 0; c < tc; ++c) {
            const T* cr = Cs + (size_t)c * d;
            const double tau = sink.tau();
            double acc = 0.0;
            for (int ax = 0; ax < d; ++ax) {
                acc = within_axis<M>(acc, (double)Qs[(size_t)ax * QB + tid], (double)cr[ax]);
                if (acc > tau) break;
            }
            if (acc <= tau) sink.offer(acc, (uint32_t)c);
        }
    }
}

// predict's sink: the smallest label among the cores within thr.
struct MinLabel {
    const int32_t* lab;
    double thr;
    int32_t best;
    __device__ __forceinline__ double tau() const { return thr; }
    __device__ __forceinline__ void offer(double, uint32_t j) {
        const int32_t l = lab[j];
        best = l < best ? l : best;
    }
};

// predict, d > kMaxDim.  The block's tail lanes sweep a zero row.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_query_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const int32_t* __restrict__ lab, uint64_t nc, int TC, double thr, int32_t* __restrict__ out,
    unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x;
    T* Qs = reinterpret_cast<T*>(smem);                                  // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                                         // [TC][d]
    int32_t* Ls = reinterpret_cast<int32_t*>(Cs + (size_t)TC * d);       // [TC]
    stage_queries<T>(Q, m, d, Qs, bad);
    MinLabel sink{Ls, thr, INT32_MAX};
    tile_sweep<T, M, true>(Xc, lab, nc, d, TC, Qs, Cs, Ls, true, sink);
    const uint64_t gi = (uint64_t)blockIdx.x * QB + threadIdx.x;
    if (gi < m) out[gi] = sink.best == INT32_MAX ? -1 : sink.best;
}

// ---------------------------------------------------------------- k-distance
// kdist(q) = the k-th smallest accumulator (pred.hpp: squared distance, or the
// cityblock sum) among the rows with acc <= thr, +inf when fewer than k qualify
// (DESIGN.md §12).  No label prunes a cell here: every candidate of the 3^(D-1)
// rows gets the exact fp64 accumulator, and what prunes is the moving bound
// tau = min(thr, k-th best so far), which only the list itself lowers.

constexpr int kKdistMaxK = 64;

// The k best accumulators of one lane, in registers: KT slots kept ascending
// by a branch-free insert (slot s takes min(old s, max(old s-1, acc)): 2 KT
// selects, every index a compile-time constant, so the list never leaves the
// VGPRs).  A k below KT starts with KT - k slots at -inf, which no insert
// moves, so the k-th best is always the last slot.
template <int KT>
struct RegList {
    double b[KT];
    double thr;
    __device__ __forceinline__ void init(int k, double thr_) {
        thr = thr_;
#pragma unroll
        for (int s = 0; s < KT; ++s) b[s] = s < KT - k ? -INFINITY : INFINITY;
    }
    __device__ __forceinline__ void offer(double acc, uint32_t) {
        // tau = min(thr, k-th best): a tie with a full list's last slot changes nothing
        if (!(acc <= thr && acc < b[KT - 1])) return;
#pragma unroll
        for (int s = KT - 1; s >= 1; --s) {
            const double hi = b[s - 1] > acc ? b[s - 1] : acc;
            b[s] = b[s] < hi ? b[s] : hi;
        }
        b[0] = b[0] < acc ? b[0] : acc;
    }
    __device__ __forceinline__ double result() const { return b[KT - 1]; }
};

// The same list in LDS for the larger k: best[slot][lane] (slot-major: the
// lanes of a wave hit distinct banks whatever slots they are at), unordered,
// with the largest entry's value and slot in registers.  Filling appends; a
// full list replaces its largest entry and rescans the k slots for the next
// one — k reads per accepted candidate, none per rejected one.
struct LdsList {
    double* my;      // this lane's slot 0
    int stride;      // lanes per block
    int k, cnt, imax;
    double thr, top; // top: largest entry so far
    __device__ __forceinline__ void init(double* base, int lane, int lanes, int k_, double thr_) {
        my = base + lane;
        stride = lanes;
        k = k_;
        cnt = 0;
        imax = 0;
        thr = thr_;
        top = -INFINITY;
    }
    __device__ __forceinline__ double tau() const { return cnt < k ? thr : top; }
    __device__ __forceinline__ void offer(double acc, uint32_t) {
        if (cnt < k) {
            if (!(acc <= thr)) return;
            my[(size_t)cnt * stride] = acc;
            if (acc >= top) {
                top = acc;
                imax = cnt;
            }
            ++cnt;
        } else if (acc < top) {
            my[(size_t)imax * stride] = acc;
            top = -INFINITY;
            for (int s = 0; s < k; ++s) {
                const double v = my[(size_t)s * stride];
                if (v > top) {
                    top = v;
                    imax = s;
                }
            }
        }
    }
    __device__ __forceinline__ double result() const { return cnt < k ? (double)INFINITY : top; }
};

// d <= 4: the shared walk into a list (the record number is not used).
// KT > 0: the list in registers (k <= KT); KT == 0: in dynamic LDS,
// k * blockDim.x doubles.
template <typename T, int D, int M, typename K, int KT>
__global__ __launch_bounds__(kBlock) void kdist_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    double thr, int k, double* __restrict__ out, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const QueryAt<T, D> q(Q, m, order, v.g, bad, blockDim.x);
    if (q.where == kPast) return;
    if (q.where != kInGrid) {
        out[q.qi] = INFINITY;
        return;
    }
    typename std::conditional<(KT > 0), RegList<(KT > 0 ? KT : 1)>, LdsList>::type list;
    if constexpr (KT > 0)
        list.init(k, thr);
    else
        list.init(reinterpret_cast<double*>(smem), (int)threadIdx.x, (int)blockDim.x, k, thr);
    walk<T, D, M>(v, q, list);
    out[q.qi] = list.result();
}

// d > kMaxDim: the tile sweep with each lane's list in LDS next to the tiles.
// The block's tail lanes sweep a zero row.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_kdist_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc, uint64_t nc, int TC,
    double thr, int k, double* __restrict__ out, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    double* Bs = reinterpret_cast<double*>(smem);            // [k][QB]
    T* Qs = reinterpret_cast<T*>(Bs + (size_t)k * QB);       // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                             // [TC][d]
    stage_queries<T>(Q, m, d, Qs, bad);
    LdsList list;
    list.init(Bs, tid, QB, k, thr);
    tile_sweep<T, M, false>(Xc, nullptr, nc, d, TC, Qs, Cs, nullptr, true, list);
    const uint64_t gi = (uint64_t)blockIdx.x * QB + (uint64_t)tid;
    if (gi < m) out[gi] = list.result();
}

__global__ __launch_bounds__(kBlock) void fill_f64_kernel(double* __restrict__ out, uint64_t m,
                                                          double v) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m) out[i] = v;
}

// ---------------------------------------------------------------- k nearest
// kneighbors(q) = the k smallest (acc, label) pairs, ascending, among the rows
// with acc <= thr; (-1, +inf) in the slots past them.  The
// k-distance walk / tiles with the label beside every accumulator.  The order
// is total, so the list's bound admits a tie with its worst entry and the label
// settles it: tau = min(thr, worst acc) is tested with <=, and only a candidate
// that passes it has its label fetched.  What a query keeps therefore depends
// on the (acc, label) pairs alone, never on the order the walk meets them in.

__device__ __forceinline__ bool pair_lt(double a, int32_t la, double b, int32_t lb) {
    return a < b || (a == b && la < lb);
}

// Slot t of query qi's row.  A slot nothing reached (or that holds an overflowed
// accumulator, which no finite cap admits) is written as (-1, +inf).
__device__ __forceinline__ void knn_store(int32_t* __restrict__ ids, double* __restrict__ accs,
                                          uint64_t qi, uint64_t m, int k, int t, double acc,
                                          int32_t l) {
    const uint64_t w = qi * (uint64_t)k + (uint64_t)t;   // m * k passes 2^31 (C2: from k = 22)
    if (!PD_OK(w < m * (uint64_t)k, 46, w)) return;
    const bool none = !(acc < INFINITY);
    ids[w] = none ? -1 : l;
    if (accs) accs[w] = none ? (double)INFINITY : acc;
}

// RegList with the label beside each accumulator: KT pairs kept ascending under
// (acc, label) by the same branch-free insert on pairs (slot s takes min(old s,
// max(old s-1, candidate))).  The KT - k padding slots hold (-inf, INT32_MIN),
// below every candidate, so no insert moves them; empty slots hold (+inf,
// INT32_MAX).  An equal pair is inserted beside its twin.
template <int KT>
struct RegPairs {
    double b[KT];
    int32_t l[KT];
    double thr;
    const int32_t* lab;   // lab[j]: candidate j's label
    __device__ __forceinline__ void init(const int32_t* lab_, int k, double thr_) {
        lab = lab_;
        thr = thr_;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            b[s] = s < KT - k ? -INFINITY : INFINITY;
            l[s] = s < KT - k ? INT32_MIN : INT32_MAX;
        }
    }
    __device__ __forceinline__ double tau() const { return thr < b[KT - 1] ? thr : b[KT - 1]; }
    // the candidate's label is read only once acc has passed tau
    __device__ __forceinline__ void offer(double acc, uint32_t j) {
        if (!(acc <= thr && acc <= b[KT - 1])) return;
        const int32_t la = lab[j];
        if (!pair_lt(acc, la, b[KT - 1], l[KT - 1])) return;
#pragma unroll
        for (int s = KT - 1; s >= 1; --s) {
            const bool lo = pair_lt(acc, la, b[s - 1], l[s - 1]);
            const double hb = lo ? b[s - 1] : acc;
            const int32_t hl = lo ? l[s - 1] : la;
            const bool take = pair_lt(hb, hl, b[s], l[s]);
            b[s] = take ? hb : b[s];
            l[s] = take ? hl : l[s];
        }
        const bool take = pair_lt(acc, la, b[0], l[0]);
        b[0] = take ? acc : b[0];
        l[0] = take ? la : l[0];
    }
    __device__ __forceinline__ void write(int32_t* __restrict__ ids, double* __restrict__ accs,
                                          uint64_t qi, uint64_t m, int k) const {
#pragma unroll
        for (int s = 0; s < KT; ++s)
            if (s >= KT - k) knn_store(ids, accs, qi, m, k, s - (KT - k), b[s], l[s]);
    }
};

// LdsList with the labels in a second slot-major array (12 bytes per slot):
// unordered, the largest PAIR's value, label and slot in registers.  A full
// list replaces its largest pair and rescans; the row is ordered at write-out
// by a selection pass over the lane's own slots (order()).
struct LdsPairs {
    double* my;       // this lane's slot 0
    int32_t* myl;
    int stride;       // lanes per block
    int k, cnt, imax;
    double thr, top;  // (top, ltop): largest pair so far
    int32_t ltop;
    const int32_t* lab;   // lab[j]: candidate j's label
    __device__ __forceinline__ void init(const int32_t* lab_, double* base, int32_t* lbase, int lane,
                                         int lanes, int k_, double thr_) {
        lab = lab_;
        my = base + lane;
        myl = lbase + lane;
        stride = lanes;
        k = k_;
        cnt = 0;
        imax = 0;
        thr = thr_;
        top = -INFINITY;
        ltop = INT32_MIN;
    }
    __device__ __forceinline__ double tau() const { return cnt < k ? thr : top; }
    __device__ __forceinline__ void offer(double acc, uint32_t j) {
        if (!(acc <= tau())) return;
        const int32_t la = lab[j];
        if (cnt < k) {
            my[(size_t)cnt * stride] = acc;
            myl[(size_t)cnt * stride] = la;
            if (!pair_lt(acc, la, top, ltop)) {
                top = acc;
                ltop = la;
                imax = cnt;
            }
            ++cnt;
        } else if (pair_lt(acc, la, top, ltop)) {
            my[(size_t)imax * stride] = acc;
            myl[(size_t)imax * stride] = la;
            top = -INFINITY;
            ltop = INT32_MIN;
            for (int s = 0; s < k; ++s) {
                const double v = my[(size_t)s * stride];
                const int32_t lv = myl[(size_t)s * stride];
                if (!pair_lt(v, lv, top, ltop)) {
                    top = v;
                    ltop = lv;
                    imax = s;
                }
            }
        }
    }
    // The selection pass, in place: slots 0 .. cnt-1 ascending, (+inf, -1) behind
    // them.  Each step takes the smallest remaining pair to slot t and moves what
    // slot t held into its place, so equal pairs are each kept.
    __device__ __forceinline__ void order() {
        for (int t = 0; t < k; ++t) {
            double bv = INFINITY;
            int32_t bl = -1;
            if (t < cnt) {
                int bs = t;
                bv = my[(size_t)t * stride];
                bl = myl[(size_t)t * stride];
                for (int s = t + 1; s < cnt; ++s) {
                    const double v = my[(size_t)s * stride];
                    const int32_t lv = myl[(size_t)s * stride];
                    if (pair_lt(v, lv, bv, bl)) {
                        bv = v;
                        bl = lv;
                        bs = s;
                    }
                }
                if (bs != t) {
                    my[(size_t)bs * stride] = my[(size_t)t * stride];
                    myl[(size_t)bs * stride] = myl[(size_t)t * stride];
                }
            }
            my[(size_t)t * stride] = bv;
            myl[(size_t)t * stride] = bl;
        }
    }
};

// d <= 4: the walk into a pair list, after the shared prologue.  KT > 0: in
// registers (k <= KT), each lane stores its own row.  KT == 0: in dynamic LDS —
// k * blockDim.x doubles, as many int32, a query number per lane — where each
// lane orders its row and the block then stores the rows side by side (C2,
// k = 10, ids + acc of all points: 80.7 -> 75.4 ms against each lane storing
// its own); those rows leave through a barrier, so no lane of that tier exits
// early.  A non-finite query and one more than a cell outside the grid keep an
// empty list: k slots of (-1, +inf).
template <typename T, int D, int M, typename K, int KT>
__global__ __launch_bounds__(kBlock) void knn_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    double thr, int k, int32_t* __restrict__ ids, double* __restrict__ accs,
    unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool kLds = KT == 0;
    const QueryAt<T, D> q(Q, m, order, v.g, bad, blockDim.x);
    if (!kLds && q.where == kPast) return;
    typename std::conditional<(KT > 0), RegPairs<(KT > 0 ? KT : 1)>, LdsPairs>::type list;
    if constexpr (KT > 0) {
        list.init(v.lab, k, thr);
    } else {
        double* Bs = reinterpret_cast<double*>(smem);
        list.init(v.lab, Bs, reinterpret_cast<int32_t*>(Bs + (size_t)k * blockDim.x),
                  (int)threadIdx.x, (int)blockDim.x, k, thr);
    }
    // The walk (for_each_row + row_run + scan_run) written out: through the
    // shared helpers the register pair lists of d = 1 lose a wave of occupancy,
    // and with only the scan written out k = 10 over all of C2 is 0.2 % slower
    // (DESIGN.md §15).  Keep it in step with them.
    if (q.where == kInGrid) {
        const IxGrid& g = v.g;
        const int64_t (&c)[D] = q.c;
        const double (&a)[D] = q.a;
        const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
        const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
        for (int rq = 0; rq < Rows<D>::v; ++rq) {
            const int r = (rq + Rows<D>::v / 2) % Rows<D>::v;
            uint64_t base = 0;
            bool in = true;
            int rr = r;
#pragma unroll
            for (int ax = D - 1; ax >= 1; --ax) {
                int pw = 1;
                for (int t = 1; t < ax; ++t) pw *= 3;
                const int64_t y = c[ax] + (int64_t)(rr / pw) - 1;
                rr %= pw;
                in = in && y >= 0 && y < g.nc[ax];
                base += (uint64_t)(in ? y : 0) * g.stride[ax];
            }
            if (!in) continue;
            const uint64_t klo = base + (uint64_t)x0, khi = base + (uint64_t)x1;
            const uint64_t b = klo >> v.shift;
            if (!PD_OK(b + 1 < v.ntab, 41, b)) continue;
            const uint32_t e0 = cell_lower_bound<K>(v.ckey, v.tab[b], v.tab[b + 1], klo);
            uint32_t e1 = e0;
            for (; e1 < v.ncells && (uint64_t)v.ckey[e1] <= khi; ++e1) {}   // <= 3 cells
            if (e1 == e0) continue;
            uint32_t j = v.cstart[e0];
            const uint32_t j1 = v.cstart[e1];
            if (!PD_OK(j <= j1 && j1 <= v.nrec, 42, j1)) continue;
            for (; j + 4 <= j1; j += 4) {
                double acc4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double bv[D];
                    load_rec<T, D>(v.Xs, j + u, bv);
                    double acc = 0.0;
#pragma unroll
                    for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                    acc4[u] = acc;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) list.offer(acc4[u], j + u);
            }
            for (; j < j1; ++j) {
                double bv[D];
                load_rec<T, D>(v.Xs, j, bv);
                double acc = 0.0;
#pragma unroll
                for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                list.offer(acc, j);
            }
        }
    }
    if constexpr (kLds) {
        // the block's rows, ordered in LDS, leave side by side: consecutive lanes
        // store consecutive slots of one row, 64 / k rows per store instruction
        const int lanes = (int)blockDim.x, tid = (int)threadIdx.x;
        double* Bs = reinterpret_cast<double*>(smem);
        int32_t* Li = reinterpret_cast<int32_t*>(Bs + (size_t)k * lanes);
        uint32_t* Qi = reinterpret_cast<uint32_t*>(Li + (size_t)k * lanes);
        list.order();
        Qi[tid] = q.where != kPast ? (uint32_t)q.qi : 0xFFFFFFFFu;   // m < 2^32 - 1
        __syncthreads();
        for (int e = tid; e < lanes * k; e += lanes) {
            const int rl = e / k, t = e - rl * k;
            const uint32_t qr = Qi[rl];
            if (qr != 0xFFFFFFFFu)
                knn_store(ids, accs, (uint64_t)qr, m, k, t, Bs[(size_t)t * lanes + rl],
                          Li[(size_t)t * lanes + rl]);
        }
    } else {
        list.write(ids, accs, q.qi, m, k);
    }
}

// d > kMaxDim: the tile sweep with the rows' labels streamed beside them and
// each lane's pair list in LDS.  A sum equal to tau runs to the end and is
// offered, where its label decides.  The block's tail lanes sweep nothing and
// write nothing.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_knn_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const int32_t* __restrict__ lab, uint64_t nc, int TC, double thr, int k,
    int32_t* __restrict__ ids, double* __restrict__ accs, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    double* Bs = reinterpret_cast<double*>(smem);                        // [k][QB]
    T* Qs = reinterpret_cast<T*>(Bs + (size_t)k * QB);                   // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                                         // [TC][d]
    int32_t* Li = reinterpret_cast<int32_t*>(Cs + (size_t)TC * d);       // [k][QB]
    int32_t* Ls = Li + (size_t)k * QB;                                   // [TC]
    stage_queries<T>(Q, m, d, Qs, bad);
    const uint64_t gi = (uint64_t)blockIdx.x * QB + (uint64_t)tid;
    const bool live = gi < m;
    LdsPairs list;
    list.init(Ls, Bs, Li, tid, QB, k, thr);
    tile_sweep<T, M, true>(Xc, lab, nc, d, TC, Qs, Cs, Ls, live, list);
    if (live) {
        list.order();
        for (int t = 0; t < k; ++t)
            knn_store(ids, accs, gi, m, k, t, Bs[(size_t)t * QB + tid], Li[(size_t)t * QB + tid]);
    }
}

// An index without rows: every slot (-1, +inf).
__global__ __launch_bounds__(kBlock) void knn_empty_kernel(int32_t* __restrict__ ids,
                                                           double* __restrict__ accs,
                                                           uint64_t total) {
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= total) return;
    ids[w] = -1;
    if (accs) accs[w] = INFINITY;
}

// ---------------------------------------------------------------- radius query
// neighbours(q) = every row with acc(q, x) <= thr, thr = fl(radius * radius)
// (cityblock: radius) for a radius <= the index's eps: the predicate of a train
// at eps = radius.  Two passes over the same candidates with the
// same exact fp64 sum (no fp32 screen: Pred's band belongs to the index's eps):
// FILL == 0 counts each query's hits, the host scans the counts into 64-bit
// offsets, and FILL == 1 (labels) / 2 (labels and accumulators) writes hit t of
// query q to off[q] + t.
//
// One query's side of either pass.  The fill trusts nothing about `off`: a hit
// is stored only inside [off[q], min(off[q + 1], cap)) — a segment that is not
// 0 <= off[q] <= off[q + 1], or that starts beyond cap, takes no store at all —
// and a query whose hit count differs from its segment's length (or whose
// segment passes cap) is tallied, so a stale or foreign offsets array ends as
// an error code, never as a stray store.
template <int FILL>
struct RadiusRow {
    double thr;
    const int32_t* lab;     // FILL: lab[j] is candidate j's label
    int32_t* ids;
    double* accs;
    uint32_t n;             // hits so far
    int64_t pos, end, lim;  // FILL: stores go to [pos, lim)
    bool ok;
    __device__ __forceinline__ void open(double thr_, const int32_t* lab_,
                                         const int64_t* __restrict__ off, int32_t* ids_,
                                         double* accs_, uint64_t qi, uint64_t m, int64_t cap) {
        thr = thr_;
        lab = lab_;
        ids = ids_;
        accs = accs_;
        n = 0;
        if constexpr (FILL > 0) {
            ok = PD_OK(qi + 1 <= m, 45, qi);
            const int64_t p = ok ? off[qi] : 0;
            end = ok ? off[qi + 1] : 0;
            ok = ok && p >= 0 && p <= end && p <= cap;
            pos = ok ? p : 0;
            lim = ok ? (end < cap ? end : cap) : 0;
        }
    }
    __device__ __forceinline__ double tau() const { return thr; }
    __device__ __forceinline__ void offer(double acc, uint32_t j) {
        if (!(acc <= thr)) return;
        if constexpr (FILL > 0) {
            const int64_t w = pos + (int64_t)n;   // pos <= cap: no overflow
            if (w < lim) {
                ids[w] = lab[j];
                if constexpr (FILL == 2) accs[w] = acc;
            }
        }
        ++n;
    }
    __device__ __forceinline__ void close(uint32_t* __restrict__ cnt, uint64_t qi, int64_t cap,
                                          unsigned long long* __restrict__ tally) {
        if constexpr (FILL == 0) {
            cnt[qi] = n;
        } else {
            if (!ok || end > cap || (int64_t)n != end - pos) atomicAdd(tally + 1, 1ull);
        }
    }
};

// d <= 4: the walk into a RadiusRow, after the shared prologue; nothing for a
// non-finite query or one more than a cell outside the grid.  Hits keep the
// walk's order, which a given index and call fix.  tally[0]: non-finite
// queries; tally[1]: see RadiusRow.
template <typename T, int D, int M, typename K, int FILL>
__global__ __launch_bounds__(kBlock) void radius_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    double thr, uint32_t* __restrict__ cnt, const int64_t* __restrict__ off,
    int32_t* __restrict__ ids, double* __restrict__ accs, int64_t cap,
    unsigned long long* __restrict__ tally) {
    const QueryAt<T, D> q(Q, m, order, v.g, tally, kBlock);
    if (q.where == kPast) return;
    RadiusRow<FILL> row;
    row.open(thr, v.lab, off, ids, accs, q.qi, m, cap);
    // The walk (for_each_row + row_run + scan_run) written out: through the
    // shared helpers the passes over all of C2 are 0.7 - 1.5 % slower (DESIGN.md
    // §15).  Keep it in step with them.
    if (q.where == kInGrid) {
        const IxGrid& g = v.g;
        const int64_t (&c)[D] = q.c;
        const double (&a)[D] = q.a;
        const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
        const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
        for (int rq = 0; rq < Rows<D>::v; ++rq) {
            const int r = (rq + Rows<D>::v / 2) % Rows<D>::v;
            uint64_t base = 0;
            bool in = true;
            int rr = r;
#pragma unroll
            for (int ax = D - 1; ax >= 1; --ax) {
                int pw = 1;
                for (int t = 1; t < ax; ++t) pw *= 3;
                const int64_t y = c[ax] + (int64_t)(rr / pw) - 1;
                rr %= pw;
                in = in && y >= 0 && y < g.nc[ax];
                base += (uint64_t)(in ? y : 0) * g.stride[ax];
            }
            if (!in) continue;
            const uint64_t klo = base + (uint64_t)x0, khi = base + (uint64_t)x1;
            const uint64_t b = klo >> v.shift;
            if (!PD_OK(b + 1 < v.ntab, 41, b)) continue;
            const uint32_t e0 = cell_lower_bound<K>(v.ckey, v.tab[b], v.tab[b + 1], klo);
            uint32_t e1 = e0;
            for (; e1 < v.ncells && (uint64_t)v.ckey[e1] <= khi; ++e1) {}   // <= 3 cells
            if (e1 == e0) continue;
            uint32_t j = v.cstart[e0];
            const uint32_t j1 = v.cstart[e1];
            if (!PD_OK(j <= j1 && j1 <= v.nrec, 42, j1)) continue;
            for (; j + 4 <= j1; j += 4) {
                double acc4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double bv[D];
                    load_rec<T, D>(v.Xs, j + u, bv);
                    double acc = 0.0;
#pragma unroll
                    for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                    acc4[u] = acc;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) row.offer(acc4[u], j + u);
            }
            for (; j < j1; ++j) {
                double bv[D];
                load_rec<T, D>(v.Xs, j, bv);
                double acc = 0.0;
#pragma unroll
                for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                row.offer(acc, j);
            }
        }
    }
    row.close(cnt, q.qi, cap, tally);
}

// d > kMaxDim: the tile sweep into a RadiusRow, the rows' labels streamed beside
// them for a fill.  The block's tail lanes sweep nothing and emit nothing.
template <typename T, int M, int FILL>
__global__ __launch_bounds__(kBlock) void dense_radius_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const int32_t* __restrict__ lab, uint64_t nc, int TC, double thr, uint32_t* __restrict__ cnt,
    const int64_t* __restrict__ off, int32_t* __restrict__ ids, double* __restrict__ accs,
    int64_t cap, unsigned long long* __restrict__ tally) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x;
    T* Qs = reinterpret_cast<T*>(smem);                                  // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                                         // [TC][d]
    int32_t* Ls = reinterpret_cast<int32_t*>(Cs + (size_t)TC * d);       // [TC]
    stage_queries<T>(Q, m, d, Qs, tally);
    const uint64_t gi = (uint64_t)blockIdx.x * QB + threadIdx.x;
    const bool live = gi < m;
    RadiusRow<FILL> row;
    row.open(thr, Ls, off, ids, accs, live ? gi : 0, m, cap);
    tile_sweep<T, M, (FILL > 0)>(Xc, lab, nc, d, TC, Qs, Cs, Ls, live, row);
    if (live) row.close(cnt, gi, cap, tally);
}

// The fill of an empty index: every segment must be empty.
__global__ __launch_bounds__(kBlock) void radius_empty_kernel(const int64_t* __restrict__ off,
                                                              uint64_t m, int64_t cap,
                                                              unsigned long long* __restrict__ tally) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    RadiusRow<1> row;
    row.open(0.0, nullptr, off, nullptr, nullptr, i, m, cap);
    row.close(nullptr, i, cap, tally);
}

// ------------------------------------------- mutual-reachability forest
// The minimum spanning forest of the DBSCAN* graph at the index's eps
// (DESIGN.md §16): edges i < j with w(i, j) = max(acc(i, j), cd[i], cd[j]) <=
// thr, cd = kdist(k), under the strict order (w, u, v) — one defined edge list.
// Borůvka: a round finds, for every row, the lightest edge to a row of another
// component (foreign_min_kernel: the index's own walk, a lane per record), takes
// the minimum per component (two atomicMin passes over the rows' bests), hooks
// the components' choices together (uf.hpp) and renames.  Components are named
// by their smallest row, in input order (comp) and in record order (comp_rec);
// ccomp[e] is the component every record of cell e is in, -1 when they differ
// (cell_label_kernel over comp_rec), and a cell in the lane's own component is
// skipped without reading its records — what makes the later rounds cheap.

// The index's records back as rows (stride D) in record order: the queries of
// the k-distance pass and of every round.  owner[label] = the record, for
// perm_check_kernel; tally[1]: labels that are no row number.
template <typename T, int D>
__global__ __launch_bounds__(kBlock) void rec_rows_kernel(const T* __restrict__ Xs,
                                                          const int32_t* __restrict__ lab,
                                                          uint64_t n, T* __restrict__ Q,
                                                          int32_t* __restrict__ owner,
                                                          unsigned long long* __restrict__ tally) {
    constexpr int S = Stride<D>::v;
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
#pragma unroll
    for (int j = 0; j < D; ++j) Q[r * D + j] = Xs[r * S + j];
    const int32_t l = lab[r];
    if (l < 0 || (uint64_t)l >= n)
        atomicAdd(tally + 1, 1ull);
    else
        owner[l] = (int32_t)r;
}

// tally[1] += the records whose label another record holds too: with none, and
// none out of range, the labels are a permutation of the row numbers (the
// index was built with labels[i] = i).
__global__ __launch_bounds__(kBlock) void perm_check_kernel(const int32_t* __restrict__ lab,
                                                            const int32_t* __restrict__ owner,
                                                            uint64_t n,
                                                            unsigned long long* __restrict__ tally) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int32_t l = lab[r];
    if (l >= 0 && (uint64_t)l < n && owner[l] != (int32_t)r) atomicAdd(tally + 1, 1ull);
}

// Core accumulators to input order; every row its own component.
__global__ __launch_bounds__(kBlock) void forest_init_kernel(
    const int32_t* __restrict__ lab, const double* __restrict__ cd_rec, uint64_t n,
    double* __restrict__ cd, uint32_t* __restrict__ par, int32_t* __restrict__ comp,
    int32_t* __restrict__ comp_rec) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int32_t i = lab[r];
    if (!PD_OK((uint64_t)(uint32_t)i < n, 48, i)) return;
    cd[i] = cd_rec[r];
    par[i] = (uint32_t)i;
    comp[i] = i;
    comp_rec[r] = i;
}

// One round's sweep.  Lane -> record r (through `order`, as every query kernel;
// Q holds the records' rows, so the query number IS the record).  A candidate j
// weighs w = max(acc, cd_i, cd_rec[j]) >= max(acc, cd_i): cd_rec[j], comp_rec[j]
// and lab[j] are read only once that lower bound does not pass the lane's best.
// The best is the minimum under (w, row of j) among the rows of other
// components — for a fixed i the order of (w, min(i, j), max(i, j)).  (inf, -1):
// no foreign row within thr, or cd_i = inf.  tally[2] / [3] (stats != 0): cells
// met / skipped by the short cut.
template <typename T, int D, int M, typename K>
__global__ __launch_bounds__(kBlock) void foreign_min_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    double thr, const double* __restrict__ cd_rec, const int32_t* __restrict__ comp_rec,
    const int32_t* __restrict__ ccomp, double* __restrict__ bw, int32_t* __restrict__ bj,
    unsigned long long* __restrict__ tally, int stats) {
    const QueryAt<T, D> q(Q, m, order, v.g, tally, kBlock);
    unsigned seen = 0, skipped = 0;
    if (q.where != kPast && PD_OK(q.qi < v.nrec, 47, q.qi)) {
        const uint32_t r = (uint32_t)q.qi;
        const double cdi = cd_rec[r];
        double best = INFINITY;
        int32_t bestj = -1;
        if (q.where == kInGrid && cdi <= thr) {
            const int32_t ci = comp_rec[r];
            auto offer = [&](double acc, uint32_t j) {
                const double lo = acc > cdi ? acc : cdi;
                if (!(acc <= thr && lo <= best)) return;
                const double cdj = cd_rec[j];
                const double w = lo > cdj ? lo : cdj;
                if (!(w <= thr && w <= best)) return;
                if (comp_rec[j] == ci) return;
                const int32_t row = v.lab[j];
                if (w < best || row < bestj) {
                    best = w;
                    bestj = row;
                }
            };
            for_each_row<D>(v.g, q.c, [&](uint64_t klo, uint64_t khi) {
                for (uint32_t e = first_cell(v, klo); e < v.ncells && (uint64_t)v.ckey[e] <= khi;
                     ++e) {
                    ++seen;
                    if (ccomp && ccomp[e] == ci) {
                        ++skipped;
                        continue;
                    }
                    uint32_t j = v.cstart[e];
                    const uint32_t j1 = v.cstart[e + 1];
                    if (!PD_OK(j <= j1 && j1 <= v.nrec, 42, j1)) continue;
                    for (; j + 4 <= j1; j += 4) {
                        double acc4[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc4[t] = rec_acc<T, D, M>(v.Xs, j + t, q.a);
#pragma unroll
                        for (int t = 0; t < 4; ++t) offer(acc4[t], j + t);
                    }
                    for (; j < j1; ++j) offer(rec_acc<T, D, M>(v.Xs, j, q.a), j);
                }
            });
        }
        bw[r] = best;
        bj[r] = bestj;
    }
    if (stats) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            seen += (unsigned)__shfl_xor((int)seen, o, 64);
            skipped += (unsigned)__shfl_xor((int)skipped, o, 64);
        }
        if ((threadIdx.x & 63) == 0 && seen) {
            atomicAdd(tally + 2, (unsigned long long)seen);
            atomicAdd(tally + 3, (unsigned long long)skipped);
        }
    }
}

// atomicMin(table[key], val) for the wave's active lanes, reduced across the
// wave first: the lanes that share the first active lane's key fold into one
// atomic, four times over, and what is left goes alone.  In cell order the late
// rounds' waves hold one or two components, so a component of 1e8 rows costs
// about n / 64 atomics on its word, not n.  Every lane of the wave must call.
__device__ __forceinline__ void wave_min_into(bool active, uint32_t key, unsigned long long val,
                                              unsigned long long* __restrict__ table,
                                              uint64_t nkeys) {
    const int lane = (int)(threadIdx.x & 63);
    for (int it = 0; it < 4; ++it) {
        const unsigned long long mask = __ballot(active);
        if (!mask) return;
        const int leader = __ffsll((long long)mask) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader, 64);
        const bool mine = active && key == k0;
        unsigned long long x = mine ? val : ~0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(x, o, 64);
            x = y < x ? y : x;
        }
        if (lane == leader && PD_OK(k0 < nkeys, 48, k0)) atomicMin(table + k0, x);
        active = active && !mine;
    }
    if (active && PD_OK(key < nkeys, 48, key)) atomicMin(table + key, val);
}

// best_w[c] = the smallest w any row of component c found (the bits of a
// non-negative double order as uint64; ~0: none).
__global__ __launch_bounds__(kBlock) void comp_min_w_kernel(
    const double* __restrict__ bw, const int32_t* __restrict__ bj,
    const int32_t* __restrict__ comp_rec, uint64_t n, unsigned long long* __restrict__ best_w) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool have = r < n && bj[r] >= 0;
    const uint32_t c = have ? (uint32_t)comp_rec[r] : 0u;
    const unsigned long long bits = have ? (unsigned long long)__double_as_longlong(bw[r]) : ~0ull;
    wave_min_into(have, c, bits, best_w, n);
}

// best_uv[c] = the smallest (u << 32 | v), u < v, among the rows of c whose w
// is best_w[c]: with it the component's choice is its minimum under (w, u, v).
__global__ __launch_bounds__(kBlock) void comp_min_uv_kernel(
    const double* __restrict__ bw, const int32_t* __restrict__ bj,
    const int32_t* __restrict__ comp_rec, const int32_t* __restrict__ lab, uint64_t n,
    const unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_uv) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool have = r < n && bj[r] >= 0;
    const uint32_t c = have ? (uint32_t)comp_rec[r] : 0u;
    unsigned long long uv = ~0ull;
    if (have) {
        have = PD_OK(c < n, 48, c) &&
               (unsigned long long)__double_as_longlong(bw[r]) == best_w[c];
        const uint32_t i = (uint32_t)lab[r], j = (uint32_t)bj[r];
        uv = i < j ? ((unsigned long long)i << 32) | j : ((unsigned long long)j << 32) | i;
    }
    wave_min_into(have, c, uv, best_uv, n);
}

// Every component with a choice unites with the component at the other end of
// it and appends the edge — once: when both ends chose the same edge, the
// smaller component does.  comp, best_w and best_uv are this round's and only
// read; the appends of a wave share one atomicAdd on the counter.
__global__ __launch_bounds__(kBlock) void forest_hook_kernel(
    const int32_t* __restrict__ comp, uint64_t n, const unsigned long long* __restrict__ best_w,
    const unsigned long long* __restrict__ best_uv, uint32_t* __restrict__ par,
    int32_t* __restrict__ eu, int32_t* __restrict__ ev, double* __restrict__ ew, uint64_t cap,
    unsigned long long* __restrict__ counter) {
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool emit = false;
    unsigned long long uv = 0, wb = 0;
    if (c < n && (uint32_t)comp[c] == (uint32_t)c && best_w[c] != ~0ull) {
        wb = best_w[c];
        uv = best_uv[c];
        const uint32_t u = (uint32_t)(uv >> 32), v = (uint32_t)uv;
        if (PD_OK(u < n && v < n, 48, uv)) {
            const uint32_t cu = (uint32_t)comp[u];
            const uint32_t c2 = cu == (uint32_t)c ? (uint32_t)comp[v] : cu;
            if (PD_OK(c2 < n, 48, c2)) {
                emit = !(best_w[c2] == wb && best_uv[c2] == uv && c2 < (uint32_t)c);
                uf_unite(par, (uint32_t)c, c2);
            }
        }
    }
    const unsigned long long mask = __ballot(emit);
    if (!mask) return;
    const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (emit) {
        const uint64_t slot = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (PD_OK(slot < cap, 49, slot) && slot < cap) {
            eu[slot] = (int32_t)(uv >> 32);
            ev[slot] = (int32_t)(uint32_t)uv;
            ew[slot] = __longlong_as_double((long long)wb);
        }
    }
}

// The new names: every row's root (the smallest row of its component).
__global__ __launch_bounds__(kBlock) void comp_refresh_kernel(uint32_t* __restrict__ par,
                                                              const int32_t* __restrict__ lab,
                                                              uint64_t n, int32_t* __restrict__ comp,
                                                              int32_t* __restrict__ comp_rec) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const uint32_t i = (uint32_t)lab[r];
    if (!PD_OK(i < n, 48, i)) return;
    const int32_t c = (int32_t)uf_find(par, i);
    comp[i] = c;
    comp_rec[r] = c;
}

// The final order (w, u, v), least significant key first: (u << 32 | v) ...
__global__ __launch_bounds__(kBlock) void edge_uv_key_kernel(const int32_t* __restrict__ eu,
                                                             const int32_t* __restrict__ ev,
                                                             uint64_t E, uint64_t* __restrict__ key,
                                                             uint32_t* __restrict__ perm) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    key[e] = ((uint64_t)(uint32_t)eu[e] << 32) | (uint32_t)ev[e];
    perm[e] = (uint32_t)e;
}

// ... then, stably, the bits of w.
__global__ __launch_bounds__(kBlock) void edge_w_key_kernel(const double* __restrict__ ew,
                                                            const uint32_t* __restrict__ perm,
                                                            uint64_t E, uint64_t* __restrict__ key) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= E) return;
    const uint32_t e = perm[t];
    key[t] = PD_OK(e < E, 49, e) ? (uint64_t)__double_as_longlong(ew[e]) : 0;
}

__global__ __launch_bounds__(kBlock) void edge_gather_kernel(
    const int32_t* __restrict__ eu, const int32_t* __restrict__ ev, const double* __restrict__ ew,
    const uint32_t* __restrict__ perm, uint64_t E, int32_t* __restrict__ u, int32_t* __restrict__ v,
    double* __restrict__ w) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= E) return;
    const uint32_t e = perm[t];
    if (!PD_OK(e < E, 49, e)) return;
    u[t] = eu[e];
    v[t] = ev[e];
    w[t] = ew[e];
}

// pd_forest_labels: the prefix's unions; tally[0]: endpoints that are no row.
__global__ __launch_bounds__(kBlock) void prefix_unite_kernel(const int32_t* __restrict__ u,
                                                              const int32_t* __restrict__ v,
                                                              uint64_t np, uint64_t n,
                                                              uint32_t* __restrict__ par,
                                                              unsigned long long* __restrict__ tally) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= np) return;
    const int32_t a = u[e], b = v[e];
    if (a < 0 || b < 0 || (uint64_t)a >= n || (uint64_t)b >= n) {
        atomicAdd(tally, 1ull);
        return;
    }
    uf_unite(par, (uint32_t)a, (uint32_t)b);
}

__global__ __launch_bounds__(kBlock) void iota_none_kernel(uint32_t* __restrict__ par,
                                                           uint32_t* __restrict__ first,
                                                           uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    par[i] = (uint32_t)i;
    first[i] = kNone;
}

// first[root] = the smallest member row of the component.
__global__ __launch_bounds__(kBlock) void first_member_kernel(uint32_t* __restrict__ par,
                                                              const uint8_t* __restrict__ member,
                                                              uint64_t n,
                                                              uint32_t* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !member[i]) return;
    atomicMin(first + uf_find(par, (uint32_t)i), (uint32_t)i);
}

// The train's cluster key: a member's component's smallest member, kNone else.
__global__ __launch_bounds__(kBlock) void member_key_kernel(uint32_t* __restrict__ par,
                                                            const uint8_t* __restrict__ member,
                                                            const uint32_t* __restrict__ first,
                                                            uint64_t n, uint32_t* __restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    key[i] = member[i] ? first[uf_find(par, (uint32_t)i)] : kNone;
}

// ------------------------------------------------------ weighted k-distance
// cdw(q) = the accumulator at which the running sum of the fixed-point weights
// W of the rows with acc <= thr and W > 0, taken ascending by acc, reaches
// T = k * 2^20; +inf when it never does.  W is the train's
// fixed point (engine.hip, weight_fix_kernel), so cdw <= thr' is the weighted
// train's core flag at every thr' <= thr.  With W_min the smallest non-zero W,
// the slots = ceil(T / W_min) smallest positive-weight candidates hold the
// crossing (their weights sum to >= slots * W_min >= T), so a list of `slots`
// (acc, weight) pairs per lane is exact, and tau = min(thr, slots-th smallest
// so far) prunes as in the unweighted lists.  A weight above T crosses wherever
// it stands, so the index keeps min(W, kWeightClamp) — 32 bits —, kWeightClamp
// = PD_KDIST_MAX_K * 2^20 >= every T; the running sum is taken in 64 bits.

constexpr int kWeightBits = 20;
constexpr double kWeightLimit = 2147483648.0;
constexpr uint32_t kWeightClamp = (uint32_t)kKdistMaxK << kWeightBits;

// The train's rule on the index's side: W = llrint(w * 2^20), valid when finite
// and 0 <= w <= 2^31, else counted in stats[0] and stored as 0; stats[2] = the
// smallest non-zero W (starts at ~0), one atomic per wave.
__global__ __launch_bounds__(kBlock) void index_weight_fix_kernel(
    const double* __restrict__ w, uint64_t n, uint64_t* __restrict__ W,
    unsigned long long* __restrict__ stats) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const double x = i < n ? w[i] : 0.0;
    const bool ok = x >= 0.0 && x <= kWeightLimit;   // (NaN fails both)
    const uint64_t Wi = ok ? (uint64_t)llrint(x * (double)(1ull << kWeightBits)) : 0ull;
    if (i < n) W[i] = Wi;
    const unsigned long long b = __ballot(!ok);
    const int lane = (int)(threadIdx.x & 63);
    if (b && lane == __ffsll((long long)b) - 1) atomicAdd(stats, (unsigned long long)__popcll(b));
    unsigned long long mn = Wi ? (unsigned long long)Wi : ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(mn, o, 64);
        mn = y < mn ? y : mn;
    }
    if (lane == 0 && mn != ~0ull) atomicMin(stats + 2, mn);
}

// wrec[r] = min(W[lab[r]], kWeightClamp): the weights in the index's own order
// (d <= 4: records; d > 4: the compacted rows).  owner[label] = r for
// perm_check_kernel; stats[1]: labels that are no row number.
__global__ __launch_bounds__(kBlock) void index_weight_gather_kernel(
    const uint64_t* __restrict__ W, const int32_t* __restrict__ lab, uint64_t n,
    uint32_t* __restrict__ wrec, int32_t* __restrict__ owner,
    unsigned long long* __restrict__ stats) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int32_t l = lab[r];
    if (l < 0 || (uint64_t)l >= n) {
        atomicAdd(stats + 1, 1ull);
        wrec[r] = 0u;
        return;
    }
    owner[l] = (int32_t)r;
    const uint64_t Wl = W[l];
    wrec[r] = Wl > (uint64_t)kWeightClamp ? kWeightClamp : (uint32_t)Wl;
}

// RegList with the weight beside each accumulator: KT pairs kept ascending by
// acc.  Slot s keeps its pair when that is <= the candidate and else takes the
// larger of the candidate and slot s - 1's pair (an equal accumulator goes
// behind its twins: every pair is kept once, whatever the ties) — 4 KT selects,
// every index a compile-time constant.  The KT - slots padding slots hold
// (-inf, 0), which no insert moves and which add nothing to the sum; empty
// slots hold (+inf, 0).  The candidate's weight is read only once acc has
// passed tau, and a zero weight is dropped there.
template <int KT>
struct WRegList {
    double b[KT];
    uint32_t wt[KT];
    double thr;
    const uint32_t* wsrc;   // wsrc[j]: candidate j's weight
    __device__ __forceinline__ void init(const uint32_t* wsrc_, int slots, double thr_) {
        wsrc = wsrc_;
        thr = thr_;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            b[s] = s < KT - slots ? -INFINITY : INFINITY;
            wt[s] = 0u;
        }
    }
    __device__ __forceinline__ double tau() const { return thr < b[KT - 1] ? thr : b[KT - 1]; }
    __device__ __forceinline__ void offer(double acc, uint32_t j) {
        // a tie with a full list's last slot changes no crossing
        if (!(acc <= thr && acc < b[KT - 1])) return;
        const uint32_t wa = wsrc[j];
        if (wa == 0u) return;
#pragma unroll
        for (int s = KT - 1; s >= 1; --s) {
            const bool stay = b[s] <= acc, up = b[s - 1] > acc;
            const double hb = up ? b[s - 1] : acc;
            const uint32_t hw = up ? wt[s - 1] : wa;
            b[s] = stay ? b[s] : hb;
            wt[s] = stay ? wt[s] : hw;
        }
        const bool stay = b[0] <= acc;
        b[0] = stay ? b[0] : acc;
        wt[0] = stay ? wt[0] : wa;
    }
    // the accumulator at which the running sum reaches `target`
    __device__ __forceinline__ double result(uint32_t target) const {
        unsigned long long sum = 0;
        double r = INFINITY;
        bool done = false;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            sum += wt[s];
            const bool hit = !done && sum >= (unsigned long long)target;
            r = hit ? b[s] : r;
            done = done || hit;
        }
        return r;
    }
};

// LdsList with the weights in a second slot-major array (12 bytes per slot):
// unordered, the largest accumulator's value and slot in registers.  The
// crossing is taken once, after the walk: the smallest entry whose own and
// smaller entries' weights sum to the target (k^2 reads per lane).
struct WLdsList {
    double* my;       // this lane's slot 0
    uint32_t* myw;
    int stride;       // lanes per block
    int k, cnt, imax;
    double thr, top;  // top: largest accumulator so far
    const uint32_t* wsrc;   // wsrc[j]: candidate j's weight
    __device__ __forceinline__ void init(const uint32_t* wsrc_, double* base, uint32_t* wbase,
                                         int lane, int lanes, int k_, double thr_) {
        wsrc = wsrc_;
        my = base + lane;
        myw = wbase + lane;
        stride = lanes;
        k = k_;
        cnt = 0;
        imax = 0;
        thr = thr_;
        top = -INFINITY;
    }
    __device__ __forceinline__ double tau() const { return cnt < k ? thr : top; }
    __device__ __forceinline__ void offer(double acc, uint32_t j) {
        if (cnt < k) {
            if (!(acc <= thr)) return;
            const uint32_t wa = wsrc[j];
            if (wa == 0u) return;
            my[(size_t)cnt * stride] = acc;
            myw[(size_t)cnt * stride] = wa;
            if (acc >= top) {
                top = acc;
                imax = cnt;
            }
            ++cnt;
        } else if (acc < top) {
            const uint32_t wa = wsrc[j];
            if (wa == 0u) return;
            my[(size_t)imax * stride] = acc;
            myw[(size_t)imax * stride] = wa;
            top = -INFINITY;
            for (int s = 0; s < k; ++s) {
                const double v = my[(size_t)s * stride];
                if (v > top) {
                    top = v;
                    imax = s;
                }
            }
        }
    }
    __device__ __forceinline__ double result(uint32_t target) const {
        double r = INFINITY;
        for (int s = 0; s < cnt; ++s) {
            const double as = my[(size_t)s * stride];
            if (!(as < r)) continue;
            unsigned long long sum = 0;
            for (int t = 0; t < cnt; ++t)
                sum += my[(size_t)t * stride] <= as ? myw[(size_t)t * stride] : 0u;
            if (sum >= (unsigned long long)target) r = as;
        }
        return r;
    }
};

// d <= 4: the shared walk into a weighted list; wrec[j] is record j's weight.
// KT > 0: the list in registers (slots <= KT); KT == 0: in dynamic LDS,
// slots * blockDim.x doubles and as many uint32.
template <typename T, int D, int M, typename K, int KT>
__global__ __launch_bounds__(kBlock) void wkdist_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxView<T, K> v,
    const uint32_t* __restrict__ wrec, double thr, int slots, uint32_t target,
    double* __restrict__ out, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const QueryAt<T, D> q(Q, m, order, v.g, bad, blockDim.x);
    if (q.where == kPast) return;
    if (q.where != kInGrid) {
        out[q.qi] = INFINITY;
        return;
    }
    typename std::conditional<(KT > 0), WRegList<(KT > 0 ? KT : 1)>, WLdsList>::type list;
    if constexpr (KT > 0) {
        list.init(wrec, slots, thr);
    } else {
        double* Bs = reinterpret_cast<double*>(smem);
        list.init(wrec, Bs, reinterpret_cast<uint32_t*>(Bs + (size_t)slots * blockDim.x),
                  (int)threadIdx.x, (int)blockDim.x, slots, thr);
    }
    walk<T, D, M>(v, q, list);
    out[q.qi] = list.result(target);
}

// d > kMaxDim: the tile sweep with the rows' weights streamed beside them
// (where predict streams labels) and each lane's weighted list in LDS.  The
// block's tail lanes sweep nothing and write nothing.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_wkdist_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const uint32_t* __restrict__ wrow, uint64_t nc, int TC, double thr, int slots,
    uint32_t target, double* __restrict__ out, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    double* Bs = reinterpret_cast<double*>(smem);                        // [slots][QB]
    T* Qs = reinterpret_cast<T*>(Bs + (size_t)slots * QB);               // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                                         // [TC][d]
    uint32_t* Wi = reinterpret_cast<uint32_t*>(Cs + (size_t)TC * d);     // [slots][QB]
    int32_t* Ws = reinterpret_cast<int32_t*>(Wi + (size_t)slots * QB);   // [TC]
    stage_queries<T>(Q, m, d, Qs, bad);
    const uint64_t gi = (uint64_t)blockIdx.x * QB + (uint64_t)tid;
    const bool live = gi < m;
    WLdsList list;
    list.init(reinterpret_cast<const uint32_t*>(Ws), Bs, Wi, tid, QB, slots, thr);
    tile_sweep<T, M, true>(Xc, reinterpret_cast<const int32_t*>(wrow), nc, d, TC, Qs, Cs, Ws, live,
                           list);
    if (live) out[gi] = list.result(target);
}

inline unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

uint64_t read_u64(Ctx& w, const unsigned long long* dev, int count, unsigned long long* host_out,
                  hipStream_t s) {
    unsigned long long* h = (unsigned long long*)pinned(w, sizeof(unsigned long long) * count);
    PD_HIP(hipMemcpyAsync(h, dev, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, s));
    sync(s);
    for (int i = 0; i < count; ++i) host_out[i] = h[i];
    return host_out[0];
}

// The grid over [lo, hi]: cells eps*(1 + 2^-20)*grow wide, grow doubled until
// every axis has <= 2^28 cells and the key stays below 2^62.
void size_grid(Index& ix, const double* lo, const double* hi) {
    const int d = ix.d;
    double grow = 1.0;
    for (int attempt = 0;; ++attempt) {
        const double cw = ix.eps * (1.0 + 1.0 / 1048576.0) * grow;
        const double inv = 1.0 / cw;
        bool ok = std::isfinite(cw) && inv > 0.0;
        long double G = 1;
        for (int j = 0; j < d && ok; ++j) {
            const double nc = std::floor((hi[j] - lo[j]) * inv) + 1.0;
            if (!(nc >= 1.0 && nc <= (double)kMaxAxisCells)) {
                ok = false;
                break;
            }
            ix.g.lo[j] = lo[j];
            ix.g.inv[j] = inv;
            ix.g.nc[j] = (int64_t)nc;
            G *= (long double)nc;
        }
        if (ok && G < 4.0e18L) {
            uint64_t st = 1;
            for (int j = 0; j < d; ++j) {
                ix.g.stride[j] = st;
                st *= (uint64_t)ix.g.nc[j];
            }
            ix.g.G = st;
            break;
        }
        if (attempt >= 2200)
            throw Error(-5, "pd_index_build: no cell size fits the cores' extent");
        grow *= 2.0;
    }
    ix.key_bits = 1;
    while (ix.key_bits < 64 && (ix.g.G >> ix.key_bits)) ++ix.key_bits;
    ix.key_bytes = ix.g.G < 0xFFFFFFFFull ? 4 : 8;
}

void drop_scratch(Index& ix) {
    ix.work.arena.release();
    ix.work.rs_look = nullptr;   // the sort's look-back words went with the arena
    ix.work.rs_look_tiles = 0;
    ix.work.rs_epoch = 0;
}

template <typename T, int D, typename K>
void build_grid(Index& ix, const T* X, const uint32_t* clist, const int32_t* labels,
                hipStream_t s) {
    constexpr int S = Stride<D>::v;
    Ctx& w = ix.work;
    const uint64_t nc = ix.nc;
    K* keys = w.arena.get<K>("ix_keys", nc);
    uint32_t* vals = w.arena.get<uint32_t>("ix_vals", nc);
    hipLaunchKernelGGL((core_key_kernel<T, D, K>), dim3(blocks(nc)), dim3(kBlock), 0, s, X, clist,
                       nc, ix.g, keys, vals);
    PD_HIP(hipGetLastError());
    sort_pairs_inplace(w, keys, (int)sizeof(K), vals, nc, ix.key_bits, s);
    T* Xs = ix.keep.get<T>("Xs", nc * S);
    ix.lab = ix.keep.get<int32_t>("lab", nc);
    hipLaunchKernelGGL((core_gather_kernel<T, D>), dim3(blocks(nc)), dim3(kBlock), 0, s, X, clist,
                       vals, labels, nc, Xs, ix.lab);
    ix.Xs = Xs;
    uint32_t* heads = w.arena.get<uint32_t>("ix_heads", nc + 1);
    const uint64_t ncells =
        compact_ordered(w, "ix_h", nc, HeadPred<K>{keys}, heads, nullptr, s);   // syncs
    ix.ncells = (uint32_t)ncells;
    ix.cstart = ix.keep.get<uint32_t>("cstart", ncells + 1);
    PD_HIP(hipMemcpyAsync(ix.cstart, heads, sizeof(uint32_t) * ncells, hipMemcpyDeviceToDevice, s));
    K* ckey = ix.keep.get<K>("ckey", ncells);
    hipLaunchKernelGGL((cell_keys_kernel<K>), dim3(blocks(ncells + 1)), dim3(kBlock), 0, s, keys,
                       ix.cstart, ix.ncells, (uint32_t)nc, ckey);
    ix.ckey = ckey;
    ix.clab = ix.keep.get<int32_t>("clab", ncells);
    hipLaunchKernelGGL(cell_label_kernel, dim3(blocks(ncells)), dim3(kBlock), 0, s, ix.cstart,
                       ix.lab, ix.ncells, ix.clab);
    // key prefixes: about two per occupied cell, 2^8 .. 2^22 of them
    int cb = 1;
    while (cb < 32 && (ncells >> cb)) ++cb;
    const int tb = std::min(22, std::max(8, cb + 1));
    int kb = 1;
    while (kb < 64 && ((ix.g.G - 1) >> kb)) ++kb;
    ix.shift = kb > tb ? kb - tb : 0;
    ix.ntab = ((ix.g.G - 1) >> ix.shift) + 2;
    ix.tab = ix.keep.get<uint32_t>("tab", ix.ntab);
    hipLaunchKernelGGL((cell_tab_kernel<K>), dim3(blocks(ix.ntab)), dim3(kBlock), 0, s, ckey,
                       ix.ncells, ix.shift, ix.ntab, ix.tab);
    PD_HIP(hipGetLastError());
}

template <typename T, typename K>
void build_grid_d(Index& ix, const T* X, const uint32_t* clist, const int32_t* labels,
                  hipStream_t s) {
    switch (ix.d) {
        case 1: build_grid<T, 1, K>(ix, X, clist, labels, s); break;
        case 2: build_grid<T, 2, K>(ix, X, clist, labels, s); break;
        case 3: build_grid<T, 3, K>(ix, X, clist, labels, s); break;
        default: build_grid<T, 4, K>(ix, X, clist, labels, s); break;
    }
}

template <typename T>
void build_t(Index& ix, const T* X, int64_t n, const uint8_t* core, const int32_t* labels,
             hipStream_t s) {
    Ctx& w = ix.work;
    const int d = ix.d;
    uint32_t* clist = w.arena.get<uint32_t>("ix_clist", (size_t)n);
    ix.nc = compact_ordered(w, "ix_c", (uint64_t)n, CorePred{core}, clist, nullptr, s);   // syncs
    if (ix.nc == 0) return;
    unsigned long long init[kStatSlots], st[kStatSlots];
    for (int i = 0; i < kStatSlots; ++i) init[i] = (i >= 2 && i < 2 + kMaxDim) ? ~0ull : 0ull;
    unsigned long long* stats = w.arena.get<unsigned long long>("ix_stats", kStatSlots);
    PD_HIP(hipMemcpyAsync(stats, init, sizeof(init), hipMemcpyHostToDevice, s));
    sync(s);   // init is a stack array
    hipLaunchKernelGGL((core_stats_kernel<T>), dim3(grid_for((int64_t)ix.nc, 1024)), dim3(kBlock),
                       0, s, X, d, clist, ix.nc, labels, stats);
    PD_HIP(hipGetLastError());
    read_u64(w, stats, kStatSlots, st, s);
    if (st[0]) throw Error(-1, "pd_index_build: a core point has a NaN or infinite coordinate");
    if (st[1]) throw Error(-1, "pd_index_build: a core point has a negative label");
    if (d > kMaxDim) {
        T* Xc = ix.keep.get<T>("Xs", ix.nc * (size_t)d);
        ix.lab = ix.keep.get<int32_t>("lab", ix.nc);
        hipLaunchKernelGGL((rows_gather_kernel<T>), dim3(blocks(ix.nc * (uint64_t)d)), dim3(kBlock),
                           0, s, X, d, clist, labels, ix.nc, Xc, ix.lab);
        PD_HIP(hipGetLastError());
        ix.Xs = Xc;
        return;
    }
    double lo[kMaxDim], hi[kMaxDim];
    for (int j = 0; j < d; ++j) {
        lo[j] = dec_f64(st[2 + j]);
        hi[j] = dec_f64(st[2 + kMaxDim + j]);
    }
    size_grid(ix, lo, hi);
    if (ix.key_bytes == 4)
        build_grid_d<T, uint32_t>(ix, X, clist, labels, s);
    else
        build_grid_d<T, uint64_t>(ix, X, clist, labels, s);
}

// The cell-sorted sweep's order of m queries (null below sort_min(): input
// order): lane i of a query kernel takes query order[i].
template <typename T, int D, typename K>
const uint32_t* query_order(Index& ix, const T* Q, uint64_t m, hipStream_t s) {
    if (m < sort_min()) return nullptr;
    Ctx& w = ix.work;
    K* keys = w.arena.get<K>("q_keys", m);
    uint32_t* vals = w.arena.get<uint32_t>("q_vals", m);
    hipLaunchKernelGGL((query_key_kernel<T, D, K>), dim3(blocks(m)), dim3(kBlock), 0, s, Q, m, ix.g,
                       keys, vals);
    PD_HIP(hipGetLastError());
    sort_pairs_inplace(w, keys, (int)sizeof(K), vals, m, ix.key_bits, s);
    return vals;
}

template <typename T, typename K>
IxView<T, K> view_of(const Index& ix) {
    return {ix.g,    (const T*)ix.Xs, ix.lab,   ix.nc,     (const K*)ix.ckey, ix.cstart,
            ix.clab, ix.tab,          ix.ntab,  ix.ncells, ix.shift};
}

// The predicate's bound on the accumulator at the index's eps.
double threshold(const Index& ix) { return ix.metric == 0 ? ix.eps * ix.eps : ix.eps; }

void check_bounds_ix(hipStream_t s, const char* kernel) {
#if PD_CHECK_BOUNDS
    sync(s);
    unsigned long long h[2] = {0, 0};
    PD_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ix_oob), sizeof(h), 0, hipMemcpyDeviceToHost));
    if (h[0]) {
        const unsigned long long z[2] = {0, 0};
        PD_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_ix_oob), z, sizeof(z), 0, hipMemcpyHostToDevice));
        throw Error(-3, std::string(kernel) + ": " + std::to_string(h[0]) +
                            " out-of-bounds accesses, first at site " + std::to_string(h[1] >> 48) +
                            " index " + std::to_string(h[1] & 0xFFFFFFFFFFFFull));
    }
#else
    (void)s;
    (void)kernel;
#endif
}

template <int V>
using Int = std::integral_constant<int, V>;
template <typename X>
struct Tag {
    using type = X;
};

// One launch of a query kernel: a lane per query, `lanes` per block; the
// arguments are the kernel's own parameter types.  Dynamic LDS beyond 64 KiB
// (the tile kernels' large plans) needs the function attribute.
template <typename... P>
void launch(void (*kernel)(P...), const char* name, uint64_t m, int lanes, size_t lds,
            hipStream_t s, typename Tag<P>::type... args) {
    if (lds > (64u << 10))
        PD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((m + lanes - 1) / lanes)), dim3(lanes), lds, s,
                       args...);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, name);
}

// From the index's run-time dtype, metric, d and key width to compile-time
// ones, as tags (std::integral_constant values, Tag<type>):
//   d <= 4: grid(Tag<T>, Int<D>, Int<M>, Tag<K>)     d > 4: tile(Tag<T>, Int<M>)
template <typename G, typename F>
void dispatch(const Index& ix, G&& grid, F&& tile) {
    auto by_d = [&](auto T, auto M) {
        auto by_key = [&](auto D) {
            if (ix.key_bytes == 4)
                grid(T, D, M, Tag<uint32_t>{});
            else
                grid(T, D, M, Tag<uint64_t>{});
        };
        switch (ix.d) {
            case 1: by_key(Int<1>{}); break;
            case 2: by_key(Int<2>{}); break;
            case 3: by_key(Int<3>{}); break;
            case 4: by_key(Int<4>{}); break;
            default: tile(T, M); break;
        }
    };
    auto by_metric = [&](auto T) {
        if (ix.metric == 0)
            by_d(T, Int<0>{});
        else
            by_d(T, Int<1>{});
    };
    if (ix.dtype == 0)
        by_metric(Tag<float>{});
    else
        by_metric(Tag<double>{});
}

// The list tier of a run-time k, f(Int<KT>, lanes per block) (DESIGN.md §12 and
// §14 have the resource reports behind it): registers up to 8 (KT slots), LDS
// above (KT = 0) with the block sized so that a block's list of doubles stays at
// 32 KiB — 256 lanes up to k = 16, 128 up to 32, 64 up to 64.  With 12 bytes per
// slot (pairs) that is at most 48 KiB and three blocks share a CU's 160 KiB: 12,
// 6 and 3 waves per CU at the top of each tier.
template <typename F>
void for_k_tier(int k, F&& f) {
    if (k <= 4)
        f(Int<4>{}, kBlock);
    else if (k <= 8)
        f(Int<8>{}, kBlock);
    else
        f(Int<0>{}, k <= 16 ? 256 : k <= 32 ? 128 : 64);
}

// The LDS plan of a tile kernel: QB lanes per block, TC rows per tile.  A lane
// holds its query row and `lane_extra` bytes (its list), a tile row the row and
// `tile_extra` bytes (its label).  The row limit is that 64 lanes of rows and
// one labelled tile row fit 60 KiB.  The block shrinks until its lanes' share is
// <= `lane_share` (never below 64 lanes); the tile takes what is left of 60 KiB,
// or, where `large` allows it and not even one tile row fits, of 144 KiB of the
// CU's 160 (through the function attribute: see launch).
struct TilePlan {
    int QB, TC;
    size_t lds;
};
TilePlan plan_tiles(const Index& ix, size_t lane_extra, size_t tile_extra, size_t lane_share,
                    bool large, const char* who) {
    const size_t row = (size_t)ix.d * (ix.dtype == 0 ? sizeof(float) : sizeof(double));
    if ((size_t)64 * row + row + 4 > (60u << 10))
        throw Error(-5, std::string(who) +
                            ": d too large for the tile kernel's LDS (d * itemsize <= 944)");
    const size_t lane = row + lane_extra, tile = row + tile_extra;
    int QB = 256;
    while (QB > 64 && (size_t)QB * lane > lane_share) QB >>= 1;
    const size_t budget =
        !large || (size_t)QB * lane + tile <= (60u << 10) ? (60u << 10) : (144u << 10);
    const int TC = (int)std::min<size_t>(64, (budget - (size_t)QB * lane) / tile);
    return {QB, TC, (size_t)QB * lane + (size_t)TC * tile};
}

// The argument checks every query entry point shares (k: only where there is one).
void check_args(const Index& ix, int dtype, int64_t m, const char* who, const int* k = nullptr) {
    const std::string w(who);
    if (k && *k < 1) throw Error(-1, w + ": k must be >= 1");
    if (k && *k > kKdistMaxK) throw Error(-5, w + ": k must be <= PD_KDIST_MAX_K (64)");
    if (dtype != ix.dtype) throw Error(-1, w + ": the queries' dtype differs from the index's");
    if (m >= 0xFFFFFFFFll) throw Error(-5, w + ": m must be < 2^32 - 1");
}

double radius_threshold(const Index& ix, int dtype, int64_t m, double radius, const char* who) {
    const std::string w(who);
    if (!(radius > 0) || !std::isfinite(radius))
        throw Error(-1, w + ": radius must be a finite value > 0");
    if (radius > ix.eps)
        throw Error(-1, w + ": radius exceeds the eps the index was built with (its cells cover "
                        "only eps)");
    check_args(ix, dtype, m, who);
    return ix.metric == 0 ? radius * radius : radius;
}

// The frame of a query call.  tally[0] counts the queries' non-finite
// coordinates — by a sweep of its own when there is nothing to walk (`empty`:
// on_empty(tally) then writes the results), by the kernels of body(tally)
// otherwise —, and the call throws if there is one.  Returns tally[1], which is
// the body's to use (both words come back in one round trip).
template <typename E, typename B>
unsigned long long run_checked(Index& ix, const void* Q, uint64_t m, bool empty, const char* who,
                               hipStream_t s, E&& on_empty, B&& body) {
    Ctx& w = ix.work;
    unsigned long long* tally = w.arena.get<unsigned long long>("q_bad", 2);
    PD_HIP(hipMemsetAsync(tally, 0, 2 * sizeof(unsigned long long), s));
    if (empty) {
        const uint64_t total = m * (uint64_t)ix.d;
        const dim3 grid(grid_for((int64_t)total, 1024));
        if (ix.dtype == 0)
            hipLaunchKernelGGL((finite_kernel<float>), grid, dim3(kBlock), 0, s, (const float*)Q,
                               total, tally);
        else
            hipLaunchKernelGGL((finite_kernel<double>), grid, dim3(kBlock), 0, s, (const double*)Q,
                               total, tally);
        PD_HIP(hipGetLastError());
        on_empty(tally);
    } else {
        body(tally);
    }
    unsigned long long* h = (unsigned long long*)pinned(w, 2 * sizeof(unsigned long long));
    PD_HIP(hipMemcpyAsync(h, tally, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    sync(s);
    if (h[0]) throw Error(-1, std::string(who) + ": a query has a NaN or infinite coordinate");
    return h[1];
}

// One pass of a radius query: the count (cnt) or a fill (off, ids, acc, cap).
struct RadiusCall {
    double thr;
    uint32_t* cnt;
    const int64_t* off;
    int32_t* ids;
    double* acc;
    int64_t cap;
    unsigned long long* tally;   // [0] non-finite queries, [1] segments that do not fit their hits
};

// Either pass over a non-empty index.  FILL: 0 the count, 1 labels, 2 labels
// and accumulators.
void radius_pass(Index& ix, const void* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    auto pass = [&](auto F) {
        constexpr int FILL = decltype(F)::value;
        dispatch(
            ix,
            [&](auto T, auto D, auto M, auto K) {
                using Tq = typename decltype(T)::type;
                using Kq = typename decltype(K)::type;
                constexpr int Dv = decltype(D)::value, Mv = decltype(M)::value;
                const uint32_t* order = query_order<Tq, Dv, Kq>(ix, (const Tq*)Q, m, s);
                launch(radius_kernel<Tq, Dv, Mv, Kq, FILL>, "radius_kernel", m, kBlock, 0, s,
                       (const Tq*)Q, m, order, view_of<Tq, Kq>(ix), rc.thr, rc.cnt, rc.off, rc.ids,
                       rc.acc, rc.cap, rc.tally);
            },
            [&](auto T, auto M) {
                using Tq = typename decltype(T)::type;
                const TilePlan p = plan_tiles(ix, 0, 4, 32u << 10, false, "pd_index_radius");
                launch(dense_radius_kernel<Tq, decltype(M)::value, FILL>, "dense_radius_kernel", m,
                       p.QB, p.lds, s, (const Tq*)Q, m, ix.d, (const Tq*)ix.Xs, ix.lab, ix.nc, p.TC,
                       rc.thr, rc.cnt, rc.off, rc.ids, rc.acc, rc.cap, rc.tally);
            });
    };
    if (!rc.off)
        pass(Int<0>{});
    else if (!rc.acc)
        pass(Int<1>{});
    else
        pass(Int<2>{});
}

// The forest's per-call switches, read like PD_INDEX_SORT_MIN.
// PD_MREACH_CELL_SKIP=0 turns the cell short cut off (same result; the A/B of
// tools/mreach_bench.py and the tests); PD_MREACH_TRACE=<file> appends one JSON
// line per round: its wall time up to the host read, the edges it emitted, the
// cells its lanes met and skipped.
bool cell_skip() {
    const char* e = std::getenv("PD_MREACH_CELL_SKIP");
    return !(e && e[0] == '0' && e[1] == 0);
}

struct Forest {
    int32_t* u;
    int32_t* v;
    double* w;
    double* cd;
    int64_t edges = 0;
    int rounds = 0;
};

template <typename T, int D, int M, typename K>
void forest_run(Index& ix, int k, bool weighted, Forest& f, hipStream_t s) {
    Ctx& w = ix.work;
    const uint64_t n = ix.nc;
    const dim3 gn(blocks(n)), bl(kBlock);
    const double thr = threshold(ix);
    // tally: [0] QueryAt's non-finite count (a record never is), [1] labels that
    // are no row number, [2] / [3] cells met / skipped, [4] the edge counter
    unsigned long long* tally = w.arena.get<unsigned long long>("mr_tally", 5);
    PD_HIP(hipMemsetAsync(tally, 0, 5 * sizeof(unsigned long long), s));
    T* Q = w.arena.get<T>("mr_q", n * D);
    int32_t* bj = w.arena.get<int32_t>("mr_bj", n);   // first: each label's record
    hipLaunchKernelGGL((rec_rows_kernel<T, D>), gn, bl, 0, s, (const T*)ix.Xs, ix.lab, n, Q, bj,
                       tally);
    hipLaunchKernelGGL(perm_check_kernel, gn, bl, 0, s, ix.lab, bj, n, tally);
    PD_HIP(hipGetLastError());
    double* cd_rec = w.arena.get<double>("mr_cd", n);
    if (weighted)   // cd = cdw: the one difference of the weighted forest
        index_kdist_weighted(&ix, Q, ix.dtype, (int64_t)n, k, cd_rec, s);
    else
        index_kdist(&ix, Q, ix.dtype, (int64_t)n, k, cd_rec, s);   // syncs
    unsigned long long h[5];
    read_u64(w, tally, 5, h, s);
    if (h[1])
        throw Error(-1, "pd_index_mreach_forest: the index's labels are not its row numbers "
                        "(build it with labels[i] = i)");
    uint32_t* par = w.arena.get<uint32_t>("mr_par", n);
    int32_t* comp = w.arena.get<int32_t>("mr_comp", n);
    int32_t* comp_rec = w.arena.get<int32_t>("mr_comp_rec", n);
    int32_t* ccomp = cell_skip() ? w.arena.get<int32_t>("mr_ccomp", ix.ncells) : nullptr;
    double* bw = w.arena.get<double>("mr_bw", n);
    unsigned long long* best_w = w.arena.get<unsigned long long>("mr_best_w", n);
    unsigned long long* best_uv = w.arena.get<unsigned long long>("mr_best_uv", n);
    const uint64_t cap = n - 1;
    int32_t* eu = w.arena.get<int32_t>("mr_eu", cap);
    int32_t* ev = w.arena.get<int32_t>("mr_ev", cap);
    double* ew = w.arena.get<double>("mr_ew", cap);
    hipLaunchKernelGGL(forest_init_kernel, gn, bl, 0, s, ix.lab, cd_rec, n, f.cd, par, comp,
                       comp_rec);
    PD_HIP(hipGetLastError());
    const uint32_t* order = query_order<T, D, K>(ix, Q, n, s);
    const char* trace = std::getenv("PD_MREACH_TRACE");
    FILE* tf = trace && *trace ? std::fopen(trace, "a") : nullptr;
    uint64_t E = 0;
    try {
        while (E < cap) {
            const auto t0 = std::chrono::steady_clock::now();
            if (ccomp)
                hipLaunchKernelGGL(cell_label_kernel, dim3(blocks(ix.ncells)), bl, 0, s, ix.cstart,
                                   comp_rec, ix.ncells, ccomp);
            if (tf) PD_HIP(hipMemsetAsync(tally + 2, 0, 2 * sizeof(unsigned long long), s));
            launch(foreign_min_kernel<T, D, M, K>, "foreign_min_kernel", n, kBlock, 0, s,
                   (const T*)Q, n, order, view_of<T, K>(ix), thr, (const double*)cd_rec,
                   (const int32_t*)comp_rec, (const int32_t*)ccomp, bw, bj, tally, tf ? 1 : 0);
            PD_HIP(hipMemsetAsync(best_w, 0xFF, sizeof(unsigned long long) * n, s));
            PD_HIP(hipMemsetAsync(best_uv, 0xFF, sizeof(unsigned long long) * n, s));
            hipLaunchKernelGGL(comp_min_w_kernel, gn, bl, 0, s, bw, bj, comp_rec, n, best_w);
            hipLaunchKernelGGL(comp_min_uv_kernel, gn, bl, 0, s, bw, bj, comp_rec, ix.lab, n,
                               best_w, best_uv);
            hipLaunchKernelGGL(forest_hook_kernel, gn, bl, 0, s, comp, n, best_w, best_uv, par, eu,
                               ev, ew, cap, tally + 4);
            hipLaunchKernelGGL(comp_refresh_kernel, gn, bl, 0, s, par, ix.lab, n, comp, comp_rec);
            PD_HIP(hipGetLastError());
            check_bounds_ix(s, "pd_index_mreach_forest");
            read_u64(w, tally, 5, h, s);   // the round's one host read
            ++f.rounds;
            const uint64_t got = h[4] - E;
            if (tf) {
                const double ms = std::chrono::duration<double, std::milli>(
                                      std::chrono::steady_clock::now() - t0).count();
                std::fprintf(tf,
                             "{\"round\": %d, \"ms\": %.3f, \"edges\": %llu, \"cells\": %llu, "
                             "\"cells_skipped\": %llu}\n",
                             f.rounds, ms, (unsigned long long)got, h[2], h[3]);
            }
            if (h[4] > cap)
                throw Error(-3, "pd_index_mreach_forest: more than n - 1 edges (a cycle)");
            if (got == 0) break;
            E = h[4];
        }
    } catch (...) {
        if (tf) std::fclose(tf);
        throw;
    }
    if (tf) std::fclose(tf);
    f.edges = (int64_t)E;
    if (E == 0) return;
    // (w, u, v) ascending: two stable passes of the record sort
    uint64_t* key = w.arena.get<uint64_t>("mr_key", E);
    uint32_t* perm = w.arena.get<uint32_t>("mr_perm", E);
    const dim3 ge(blocks(E));
    hipLaunchKernelGGL(edge_uv_key_kernel, ge, bl, 0, s, eu, ev, E, key, perm);
    int nb = 1;
    while (nb < 32 && ((n - 1) >> nb)) ++nb;
    sort_pairs_inplace(w, key, 8, perm, E, 32 + nb, s);
    hipLaunchKernelGGL(edge_w_key_kernel, ge, bl, 0, s, ew, perm, E, key);
    sort_pairs_inplace(w, key, 8, perm, E, 63, s);
    hipLaunchKernelGGL(edge_gather_kernel, ge, bl, 0, s, eu, ev, ew, perm, E, f.u, f.v, f.w);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "pd_index_mreach_forest");
    sync(s);
}

}  // namespace

namespace {
void mreach_forest(Index* ix, int k, bool weighted, int32_t* u, int32_t* v, double* w, double* cd,
                   int64_t capacity, int64_t* n_edges_host, int32_t* rounds_host, hipStream_t s) {
    const char* who = weighted ? "pd_index_mreach_forest_weighted" : "pd_index_mreach_forest";
    if (n_edges_host) *n_edges_host = 0;
    if (rounds_host) *rounds_host = 0;
    if (k < 1) throw Error(-1, std::string(who) + ": k must be >= 1");
    if (k > kKdistMaxK) throw Error(-5, std::string(who) + ": k must be <= PD_KDIST_MAX_K (64)");
    if (ix->d > kMaxDim)
        throw Error(-5, std::string(who) + ": d = " + std::to_string(ix->d) +
                            " is not supported: the forest needs the cell grid of d <= 4");
    const uint64_t n = ix->nc;
    if (n > 0x7FFFFFFFull) throw Error(-5, std::string(who) + ": n must be <= 2^31 - 1");
    if (capacity < 0 || (uint64_t)capacity + 1 < n)
        throw Error(-1, std::string(who) + ": capacity must be >= n - 1");
    if (n == 0) return;
    if (!cd || (n > 1 && (!u || !v || !w))) throw Error(-1, std::string(who) + ": null output");
    Forest f{u, v, w, cd};
    dispatch(
        *ix,
        [&](auto T, auto D, auto M, auto K) {
            forest_run<typename decltype(T)::type, decltype(D)::value, decltype(M)::value,
                       typename decltype(K)::type>(*ix, k, weighted, f, s);
        },
        [&](auto, auto) { throw Error(-5, std::string(who) + ": d > 4"); });
    if (n_edges_host) *n_edges_host = f.edges;
    if (rounds_host) *rounds_host = f.rounds;
}
}  // namespace

void index_mreach_forest(Index* ix, int k, int32_t* u, int32_t* v, double* w, double* cd,
                         int64_t capacity, int64_t* n_edges_host, int32_t* rounds_host,
                         hipStream_t s) {
    mreach_forest(ix, k, false, u, v, w, cd, capacity, n_edges_host, rounds_host, s);
}

void index_mreach_forest_weighted(Index* ix, int k, int32_t* u, int32_t* v, double* w, double* cd,
                                  int64_t capacity, int64_t* n_edges_host, int32_t* rounds_host,
                                  hipStream_t s) {
    if (n_edges_host) *n_edges_host = 0;
    if (rounds_host) *rounds_host = 0;
    if (!ix->weighted)
        throw Error(-1, "pd_index_mreach_forest_weighted: the index has no weights "
                        "(pd_index_set_weights)");
    mreach_forest(ix, k, true, u, v, w, cd, capacity, n_edges_host, rounds_host, s);
}

// Labels of the cut: the components of the first n_prefix edges, on the member
// rows, numbered by smallest member row (rank_labels: the train's numbering).
int64_t forest_labels(Ctx& ctx, int64_t n, const int32_t* u, const int32_t* v, int64_t n_prefix,
                      const uint8_t* member, int32_t* labels, hipStream_t s) {
    if (n == 0) return 0;
    const uint64_t un = (uint64_t)n, np = (uint64_t)n_prefix;
    const dim3 gn(blocks(un)), bl(kBlock);
    uint32_t* par = ctx.arena.get<uint32_t>("fl_par", un);
    uint32_t* first = ctx.arena.get<uint32_t>("fl_first", un);
    uint32_t* key = ctx.arena.get<uint32_t>("fl_key", un);
    unsigned long long* tally = ctx.arena.get<unsigned long long>("fl_tally", 1);
    PD_HIP(hipMemsetAsync(tally, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(iota_none_kernel, gn, bl, 0, s, par, first, un);
    if (np)
        hipLaunchKernelGGL(prefix_unite_kernel, dim3(blocks(np)), bl, 0, s, u, v, np, un, par,
                           tally);
    hipLaunchKernelGGL(first_member_kernel, gn, bl, 0, s, par, member, un, first);
    hipLaunchKernelGGL(member_key_kernel, gn, bl, 0, s, par, member, (const uint32_t*)first, un,
                       key);
    PD_HIP(hipGetLastError());
    rank_labels_async(ctx, key, un, labels, s);
    const int64_t ncl = rank_labels_count(ctx, s);   // syncs
    unsigned long long bad = 0;
    read_u64(ctx, tally, 1, &bad, s);
    if (bad) throw Error(-1, "pd_forest_labels: an edge's endpoint is not a row number");
    return ncl;
}

Index* index_build(int device, const void* X, int dtype, int64_t n, int d, const uint8_t* core,
                   const int32_t* labels, double eps, int metric, hipStream_t s) {
    if (!(eps > 0) || !std::isfinite(eps)) throw Error(-1, "eps must be a finite value > 0");
    if (metric != 0 && metric != 1) throw Error(-1, "metric must be 0 (euclidean) or 1 (cityblock)");
    if (dtype != 0 && dtype != 1) throw Error(-1, "dtype must be 0 (float32) or 1 (float64)");
    if (n >= 0xFFFFFFFFll) throw Error(-5, "pd_index_build: n must be < 2^32 - 1");
    Index* ix = new Index();
    ix->device = ix->work.device = device;
    ix->dtype = dtype;
    ix->d = d;
    ix->metric = metric;
    ix->eps = eps;
    ix->n_rows = (uint64_t)n;
    // fp32 screening band (see Pred): thresholds rounded outward
    const double thr = metric == 0 ? eps * eps : eps;
    if (dtype == 0 && thr > 1e-30 && thr < 1e30) {
        ix->slo = std::nextafter((float)(thr * (1.0 - 1.0 / 262144.0)), 0.0f);
        ix->shi = std::nextafter((float)(thr * (1.0 + 1.0 / 262144.0)), INFINITY);
    }
    try {
        if (n > 0) {
            if (dtype == 0)
                build_t<float>(*ix, (const float*)X, n, core, labels, s);
            else
                build_t<double>(*ix, (const double*)X, n, core, labels, s);
            sync(s);   // the scratch is freed next
        }
        drop_scratch(*ix);
    } catch (...) {
        index_destroy(ix);
        throw;
    }
    return ix;
}

void index_query(Index* ix, const void* Q, int dtype, int64_t m, int32_t* out, hipStream_t s) {
    check_args(*ix, dtype, m, "pd_index_query");
    if (m == 0) return;
    const uint64_t um = (uint64_t)m;
    run_checked(
        *ix, Q, um, ix->nc == 0, "pd_index_query", s,
        [&](unsigned long long*) {
            PD_HIP(hipMemsetAsync(out, 0xFF, sizeof(int32_t) * um, s));   // -1
        },
        [&](unsigned long long* bad) {
            dispatch(
                *ix,
                [&](auto T, auto D, auto M, auto K) {
                    using Tq = typename decltype(T)::type;
                    using Kq = typename decltype(K)::type;
                    constexpr int Dv = decltype(D)::value, Mv = decltype(M)::value;
                    const uint32_t* order = query_order<Tq, Dv, Kq>(*ix, (const Tq*)Q, um, s);
                    launch(query_kernel<Tq, Dv, Mv, Kq>, "query_kernel", um, kBlock, 0, s,
                           (const Tq*)Q, um, order, view_of<Tq, Kq>(*ix), ix->eps,
                           ix->eps * ix->eps, ix->slo, ix->shi, out, bad);
                },
                [&](auto T, auto M) {
                    using Tq = typename decltype(T)::type;
                    const TilePlan p = plan_tiles(*ix, 0, 4, 32u << 10, false, "pd_index_query");
                    launch(dense_query_kernel<Tq, decltype(M)::value>, "dense_query_kernel", um,
                           p.QB, p.lds, s, (const Tq*)Q, um, ix->d, (const Tq*)ix->Xs, ix->lab,
                           ix->nc, p.TC, threshold(*ix), out, bad);
                });
        });
}

void index_kdist(Index* ix, const void* Q, int dtype, int64_t m, int k, double* out,
                 hipStream_t s) {
    check_args(*ix, dtype, m, "pd_index_kdist", &k);
    if (m == 0) return;
    const uint64_t um = (uint64_t)m;
    const double thr = threshold(*ix);
    run_checked(
        *ix, Q, um, ix->nc < (uint64_t)k,   // fewer than k rows in all (also: an empty index)
        "pd_index_kdist", s,
        [&](unsigned long long*) {
            hipLaunchKernelGGL(fill_f64_kernel, dim3(blocks(um)), dim3(kBlock), 0, s, out, um,
                               (double)INFINITY);
            PD_HIP(hipGetLastError());
        },
        [&](unsigned long long* bad) {
            dispatch(
                *ix,
                [&](auto T, auto D, auto M, auto K) {
                    using Tq = typename decltype(T)::type;
                    using Kq = typename decltype(K)::type;
                    constexpr int Dv = decltype(D)::value, Mv = decltype(M)::value;
                    const uint32_t* order = query_order<Tq, Dv, Kq>(*ix, (const Tq*)Q, um, s);
                    for_k_tier(k, [&](auto KT, int lanes) {
                        constexpr int KTv = decltype(KT)::value;
                        const size_t lds = KTv > 0 ? 0 : (size_t)k * lanes * sizeof(double);
                        launch(kdist_kernel<Tq, Dv, Mv, Kq, KTv>, "kdist_kernel", um, lanes, lds, s,
                               (const Tq*)Q, um, order, view_of<Tq, Kq>(*ix), thr, k, out, bad);
                    });
                },
                [&](auto T, auto M) {
                    using Tq = typename decltype(T)::type;
                    const TilePlan p = plan_tiles(*ix, (size_t)k * sizeof(double), 0, 48u << 10,
                                                  true, "pd_index_kdist");
                    launch(dense_kdist_kernel<Tq, decltype(M)::value>, "dense_kdist_kernel", um,
                           p.QB, p.lds, s, (const Tq*)Q, um, ix->d, (const Tq*)ix->Xs, ix->nc, p.TC,
                           thr, k, out, bad);
                });
        });
}

// The rows' weights for pd_index_kdist_weighted and the weighted forest: the
// train's fixed point and validity rule, gathered into the index's own order.
// One host read: invalid weights, labels that are no permutation of the row
// numbers, the smallest non-zero weight.
void index_set_weights(Index* ix, const double* weight, hipStream_t s) {
    const char* who = "pd_index_set_weights";
    const uint64_t n = ix->nc;
    if (n != ix->n_rows)
        throw Error(-1, std::string(who) + ": the index must hold every row (build it with "
                                           "core = ones and labels[i] = i)");
    if (n > 0x7FFFFFFFull) throw Error(-5, std::string(who) + ": n must be <= 2^31 - 1");
    ix->weighted = false;   // until the new weights are known to be good
    ix->wmin = 0;
    if (n == 0) {
        ix->weighted = true;
        return;
    }
    if (!weight) throw Error(-1, std::string(who) + ": null sample_weight");
    Ctx& w = ix->work;
    const dim3 gn(blocks(n)), bl(kBlock);
    uint64_t* W = w.arena.get<uint64_t>("sw_fix", n);
    int32_t* owner = w.arena.get<int32_t>("sw_owner", n);
    unsigned long long* stats = w.arena.get<unsigned long long>("sw_stats", 3);
    ix->wrec = ix->keep.get<uint32_t>("wrec", n);
    PD_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s));
    PD_HIP(hipMemsetAsync(stats + 2, 0xFF, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(index_weight_fix_kernel, gn, bl, 0, s, weight, n, W, stats);
    hipLaunchKernelGGL(index_weight_gather_kernel, gn, bl, 0, s, (const uint64_t*)W, ix->lab, n,
                       ix->wrec, owner, stats);
    hipLaunchKernelGGL(perm_check_kernel, gn, bl, 0, s, ix->lab, (const int32_t*)owner, n, stats);
    PD_HIP(hipGetLastError());
    unsigned long long h[3];
    read_u64(w, stats, 3, h, s);   // syncs
    if (h[1])
        throw Error(-1, std::string(who) + ": the index's labels are not its row numbers (build "
                                           "it with labels[i] = i)");
    if (h[0])
        throw Error(-1, "sample_weight: " + std::to_string(h[0]) +
                            " value(s) not finite or outside [0, 2^31]");
    ix->wmin = h[2] == ~0ull ? 0 : (uint64_t)h[2];
    ix->weighted = true;
}

// pd_index_kdist's twin over the weights.  No short cut for an index with fewer
// than k rows: one heavy row can be enough.  Without a positive weight nothing
// ever crosses: every query gets +inf.
void index_kdist_weighted(Index* ix, const void* Q, int dtype, int64_t m, int k, double* out,
                          hipStream_t s) {
    const char* who = "pd_index_kdist_weighted";
    check_args(*ix, dtype, m, who, &k);
    if (!ix->weighted)
        throw Error(-1, std::string(who) + ": the index has no weights (pd_index_set_weights)");
    const uint64_t target = (uint64_t)k << kWeightBits;
    const uint64_t nslots = ix->wmin ? (target + ix->wmin - 1) / ix->wmin : 1;
    if (nslots > (uint64_t)kKdistMaxK)
        throw Error(-5, std::string(who) + ": min_samples = " + std::to_string(k) +
                            " with the smallest positive sample_weight " +
                            std::to_string((double)ix->wmin / (double)(1u << kWeightBits)) +
                            " needs a list of " + std::to_string(nslots) +
                            " slots per query; the limit is 64 (PD_KDIST_MAX_K)");
    if (m == 0) return;
    const uint64_t um = (uint64_t)m;
    const int slots = (int)nslots;
    const double thr = threshold(*ix);
    constexpr size_t kSlot = sizeof(double) + sizeof(uint32_t);   // a pair
    run_checked(
        *ix, Q, um, ix->nc == 0 || ix->wmin == 0, who, s,
        [&](unsigned long long*) {
            hipLaunchKernelGGL(fill_f64_kernel, dim3(blocks(um)), dim3(kBlock), 0, s, out, um,
                               (double)INFINITY);
            PD_HIP(hipGetLastError());
        },
        [&](unsigned long long* bad) {
            dispatch(
                *ix,
                [&](auto T, auto D, auto M, auto K) {
                    using Tq = typename decltype(T)::type;
                    using Kq = typename decltype(K)::type;
                    constexpr int Dv = decltype(D)::value, Mv = decltype(M)::value;
                    const uint32_t* order = query_order<Tq, Dv, Kq>(*ix, (const Tq*)Q, um, s);
                    for_k_tier(slots, [&](auto KT, int lanes) {
                        constexpr int KTv = decltype(KT)::value;
                        const size_t lds = KTv > 0 ? 0 : (size_t)slots * lanes * kSlot;
                        launch(wkdist_kernel<Tq, Dv, Mv, Kq, KTv>, "wkdist_kernel", um, lanes, lds,
                               s, (const Tq*)Q, um, order, view_of<Tq, Kq>(*ix),
                               (const uint32_t*)ix->wrec, thr, slots, (uint32_t)target, out, bad);
                    });
                },
                [&](auto T, auto M) {
                    using Tq = typename decltype(T)::type;
                    const TilePlan p = plan_tiles(*ix, (size_t)slots * kSlot, 4, 48u << 10, true,
                                                  who);
                    launch(dense_wkdist_kernel<Tq, decltype(M)::value>, "dense_wkdist_kernel", um,
                           p.QB, p.lds, s, (const Tq*)Q, um, ix->d, (const Tq*)ix->Xs,
                           (const uint32_t*)ix->wrec, ix->nc, p.TC, thr, slots, (uint32_t)target,
                           out, bad);
                });
        });
}

// No short cut for an index with fewer than k rows: the walk returns the rows
// there are.  An index without rows has nothing to walk.
void index_kneighbors(Index* ix, const void* Q, int dtype, int64_t m, int k, int32_t* ids,
                      double* acc, hipStream_t s) {
    check_args(*ix, dtype, m, "pd_index_kneighbors", &k);
    if (m == 0) return;
    const uint64_t um = (uint64_t)m;
    const double thr = threshold(*ix);
    constexpr size_t kSlot = sizeof(double) + sizeof(int32_t);   // a pair
    run_checked(
        *ix, Q, um, ix->nc == 0, "pd_index_kneighbors", s,
        [&](unsigned long long*) {
            hipLaunchKernelGGL(knn_empty_kernel, dim3(blocks(um * (uint64_t)k)), dim3(kBlock), 0, s,
                               ids, acc, um * (uint64_t)k);
            PD_HIP(hipGetLastError());
        },
        [&](unsigned long long* bad) {
            dispatch(
                *ix,
                [&](auto T, auto D, auto M, auto K) {
                    using Tq = typename decltype(T)::type;
                    using Kq = typename decltype(K)::type;
                    constexpr int Dv = decltype(D)::value, Mv = decltype(M)::value;
                    const uint32_t* order = query_order<Tq, Dv, Kq>(*ix, (const Tq*)Q, um, s);
                    for_k_tier(k, [&](auto KT, int lanes) {
                        constexpr int KTv = decltype(KT)::value;
                        // the LDS list: k pairs per lane and, for the write-out, the
                        // lane's query number
                        const size_t lds =
                            KTv > 0 ? 0 : (size_t)lanes * (k * kSlot + sizeof(uint32_t));
                        launch(knn_kernel<Tq, Dv, Mv, Kq, KTv>, "knn_kernel", um, lanes, lds, s,
                               (const Tq*)Q, um, order, view_of<Tq, Kq>(*ix), thr, k, ids, acc, bad);
                    });
                },
                [&](auto T, auto M) {
                    using Tq = typename decltype(T)::type;
                    // at most 64 * (944 + 768) = 107 KiB of lanes, which leaves 39
                    // tile rows of 948 bytes
                    const TilePlan p = plan_tiles(*ix, (size_t)k * kSlot, 4, 48u << 10, true,
                                                  "pd_index_kneighbors");
                    launch(dense_knn_kernel<Tq, decltype(M)::value>, "dense_knn_kernel", um, p.QB,
                           p.lds, s, (const Tq*)Q, um, ix->d, (const Tq*)ix->Xs, ix->lab, ix->nc,
                           p.TC, thr, k, ids, acc, bad);
                });
        });
}

// An empty index only checks the queries (and, for a fill, that every segment
// is empty).
void index_radius_count(Index* ix, const void* Q, int dtype, int64_t m, double radius,
                        int64_t* offsets, int64_t* total_host, hipStream_t s) {
    RadiusCall rc{};
    rc.thr = radius_threshold(*ix, dtype, m, radius, "pd_index_radius_count");
    if (total_host) *total_host = 0;
    if (m == 0 || ix->nc == 0)
        PD_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t) * ((size_t)m + 1), s));
    if (m == 0) return;
    Ctx& w = ix->work;
    const uint64_t um = (uint64_t)m;
    // the total rides the frame's round trip as tally[1] (0 for an empty index)
    const unsigned long long total = run_checked(
        *ix, Q, um, ix->nc == 0, "pd_index_radius_count", s, [](unsigned long long*) {},
        [&](unsigned long long* tally) {
            rc.tally = tally;
            rc.cnt = w.arena.get<uint32_t>("r_cnt", um + 1);
            PD_HIP(hipMemsetAsync(rc.cnt + um, 0, sizeof(uint32_t), s));
            radius_pass(*ix, Q, um, rc, s);
            // 32-bit counts, 64-bit sums: the total passes 2^32 long before n does
            uint64_t* off = reinterpret_cast<uint64_t*>(offsets);
            size_t tb = 0;
            PD_HIP(rocprim::exclusive_scan(nullptr, tb, rc.cnt, off, (uint64_t)0, (size_t)um + 1,
                                           rocprim::plus<uint64_t>(), s));
            void* tmp = w.arena.get<char>("r_scan_tmp", tb);
            PD_HIP(rocprim::exclusive_scan(tmp, tb, rc.cnt, off, (uint64_t)0, (size_t)um + 1,
                                           rocprim::plus<uint64_t>(), s));
            PD_HIP(hipMemcpyAsync(tally + 1, offsets + um, sizeof(int64_t),
                                  hipMemcpyDeviceToDevice, s));
        });
    if (total_host) *total_host = (int64_t)total;
}

void index_radius_fill(Index* ix, const void* Q, int dtype, int64_t m, double radius,
                       const int64_t* offsets, int32_t* ids, double* acc, int64_t capacity,
                       hipStream_t s) {
    RadiusCall rc{};
    rc.thr = radius_threshold(*ix, dtype, m, radius, "pd_index_radius_fill");
    if (capacity < 0) throw Error(-1, "pd_index_radius_fill: capacity < 0");
    if (m == 0) return;
    const uint64_t um = (uint64_t)m;
    rc.off = offsets;
    rc.ids = ids;
    rc.acc = acc;
    rc.cap = capacity;
    const unsigned long long misfits = run_checked(
        *ix, Q, um, ix->nc == 0, "pd_index_radius_fill", s,
        [&](unsigned long long* tally) {
            hipLaunchKernelGGL(radius_empty_kernel, dim3(blocks(um)), dim3(kBlock), 0, s, offsets,
                               um, capacity, tally);
            PD_HIP(hipGetLastError());
        },
        [&](unsigned long long* tally) {
            rc.tally = tally;
            radius_pass(*ix, Q, um, rc, s);
        });
    if (misfits)
        throw Error(-1, "pd_index_radius_fill: " + std::to_string(misfits) + " queries' hits do not "
                        "fit their segments: Q, radius or offsets changed since the count");
}

void index_destroy(Index* ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();   // a query may still read the buffers
    ix->keep.release();
    ix->work.arena.release();
    if (ix->work.pinned) (void)hipHostFree(ix->work.pinned);
    delete ix;
}

int index_device(const Index* ix) { return ix->device; }
int64_t index_cores(const Index* ix) { return (int64_t)ix->nc; }

}  // namespace pd
