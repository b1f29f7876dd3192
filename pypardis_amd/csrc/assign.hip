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
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "compact.hpp"
#include "internal.hpp"
#include "pred.hpp"

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

// One lane per query: the 3^(D-1) neighbour rows, the query's own first, each
// one key run of <= 3 occupied cells; fp32 screen + exact fp64 recheck (Pred)
// of the cores whose label could lower the answer; the smallest label among
// the hits.  order (nullable): lane i sweeps query
// order[i] (the queries sorted by cell), results go back to input order.
template <typename T, int D, int M, typename K>
__global__ __launch_bounds__(kBlock) void query_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxGrid g,
    const T* __restrict__ Xs, const int32_t* __restrict__ lab, const K* __restrict__ ckey,
    const uint32_t* __restrict__ cstart, const int32_t* __restrict__ clab,
    const uint32_t* __restrict__ tab, uint32_t ncells, int shift, double eps, double eps2, float slo, float shi, int32_t* __restrict__ out,
    unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint64_t qi = order ? (uint64_t)order[i] : i;
    Pred<T, D, M> pr;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        pr.ar[j] = Q[qi * D + j];
        pr.a[j] = (double)pr.ar[j];
        fin = fin && isfinite(pr.a[j]);
    }
    pr.eps = eps;
    pr.eps2 = eps2;
    pr.lo = slo;
    pr.hi = shi;
    if (!fin) {
        atomicAdd(bad, 1ull);
        out[qi] = -1;
        return;
    }
    int64_t c[D];
    if (!cell_of<D>(pr.a, g, c)) {   // outside the cores' box grown by a cell
        out[qi] = -1;
        return;
    }
    const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
    const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
    int32_t best = INT32_MAX;
    for (int rq = 0; rq < Rows<D>::v; ++rq) {
        // the query's own row first: its first hit usually settles every cell
        // of the same cluster
        const int r = (rq + Rows<D>::v / 2) % Rows<D>::v;
        uint64_t base = 0;
        bool ok = true;
        int rr = r;
#pragma unroll
        for (int a = D - 1; a >= 1; --a) {
            // r in base 3, axis D-1 the most significant digit
            int pw = 1;
            for (int t = 1; t < a; ++t) pw *= 3;
            const int64_t y = c[a] + (int64_t)(rr / pw) - 1;
            rr %= pw;
            ok = ok && y >= 0 && y < g.nc[a];
            base += (uint64_t)(ok ? y : 0) * g.stride[a];
        }
        if (!ok) continue;
        const uint64_t klo = base + (uint64_t)x0, khi = base + (uint64_t)x1;
        const uint64_t b = klo >> shift;
        uint32_t e = cell_lower_bound<K>(ckey, tab[b], tab[b + 1], klo);
        for (; e < ncells && (uint64_t)ckey[e] <= khi; ++e) {   // <= 3 cells
            const int32_t cl = clab[e];
            const uint32_t j1 = cstart[e + 1];
            uint32_t j = cstart[e];
            if (cl >= 0) {
                if (cl >= best) continue;
                for (; j < j1; ++j) {
                    T bv[D];
                    load_raw<T, D>(Xs, j, bv);
                    if (pr(bv)) {
                        best = cl;
                        break;
                    }
                }
            } else {
                for (; j < j1; ++j) {
                    const int32_t l = lab[j];
                    if (l >= best) continue;
                    T bv[D];
                    load_raw<T, D>(Xs, j, bv);
                    if (pr(bv)) best = l;
                }
            }
        }
    }
    out[qi] = best == INT32_MAX ? -1 : best;
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

// d > kMaxDim.  A block of QB lanes owns QB queries, kept transposed in LDS
// (Qs[k][lane]: conflict-free); the core rows pass through LDS in tiles of TC
// (every lane reads the same core element: a broadcast).  Each pair runs the
// predicate's own fp64 sum in axis order (within_axis) and stops at the first
// partial sum above the threshold — the sum never decreases, so the outcome is
// that of the full sum.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_query_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const int32_t* __restrict__ lab, uint64_t nc, int TC, double thr, int32_t* __restrict__ out,
    unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    T* Qs = reinterpret_cast<T*>(smem);
    T* Cs = Qs + (size_t)d * QB;
    int32_t* Ls = reinterpret_cast<int32_t*>(Cs + (size_t)TC * d);
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
    int32_t best = INT32_MAX;
    for (uint64_t t0 = 0; t0 < nc; t0 += (uint64_t)TC) {
        const int tc = (int)(nc - t0 < (uint64_t)TC ? nc - t0 : (uint64_t)TC);
        __syncthreads();
        for (int e = tid; e < tc * d; e += QB) Cs[e] = Xc[t0 * (uint64_t)d + e];
        for (int e = tid; e < tc; e += QB) Ls[e] = lab[t0 + e];
        __syncthreads();
        for (int c = 0; c < tc; ++c) {
            const T* cr = Cs + (size_t)c * d;
            double acc = 0.0;
            for (int k = 0; k < d; ++k) {
                acc = within_axis<M>(acc, (double)Qs[(size_t)k * QB + tid], (double)cr[k]);
                if (acc > thr) break;
            }
            if (acc <= thr) {
                const int32_t l = Ls[c];
                best = l < best ? l : best;
            }
        }
    }
    const uint64_t gi = q0 + (uint64_t)tid;
    if (gi < m) out[gi] = best == INT32_MAX ? -1 : best;
}

// ---------------------------------------------------------------- k-distance
// kdist(q) = the k-th smallest accumulator (pred.hpp: squared distance, or the
// cityblock sum) among the rows with acc <= thr, +inf when fewer than k qualify
// (DESIGN.md §12).  No label prunes a cell here: every candidate of the 3^(D-1)
// rows gets the exact fp64 accumulator, and what prunes is the moving bound
// tau = min(thr, k-th best so far), which only the list itself lowers.

// Device-side bounds checks of the k-distance kernels, engine.hip's scheme
// (-DPD_CHECK_BOUNDS=1 builds): a checked access that would leave its buffer
// is skipped and the first one recorded; the host reads the record after the
// kernel and throws.  Off (the default) PD_OK is `true` and costs nothing.
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
    __device__ __forceinline__ void offer(double acc) {
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
    __device__ __forceinline__ void offer(double acc) {
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

// One lane per query, query_kernel's row walk (own row first, each row one key
// run of <= 3 occupied cells, `order` for the sorted sweep, the same treatment
// of queries outside the grid).  KT > 0: the list in registers (k <= KT);
// KT == 0: in dynamic LDS, k * blockDim.x doubles.
template <typename T, int D, int M, typename K, int KT>
__global__ __launch_bounds__(kBlock) void kdist_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxGrid g,
    const T* __restrict__ Xs, uint64_t nrec, const K* __restrict__ ckey,
    const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ tab, uint64_t ntab,
    uint32_t ncells, int shift, double thr, int k, double* __restrict__ out,
    unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t qi = order ? (uint64_t)order[i] : i;
    if (!PD_OK(qi < m, 40, qi)) return;
    double a[D];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        a[j] = (double)Q[qi * D + j];
        fin = fin && isfinite(a[j]);
    }
    if (!fin) {
        atomicAdd(bad, 1ull);
        out[qi] = INFINITY;
        return;
    }
    int64_t c[D];
    if (!cell_of<D>(a, g, c)) {   // more than a cell outside the rows' box
        out[qi] = INFINITY;
        return;
    }
    typename std::conditional<(KT > 0), RegList<(KT > 0 ? KT : 1)>, LdsList>::type list;
    if constexpr (KT > 0)
        list.init(k, thr);
    else
        list.init(reinterpret_cast<double*>(smem), (int)threadIdx.x, (int)blockDim.x, k, thr);
    const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
    const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
    for (int rq = 0; rq < Rows<D>::v; ++rq) {
        // the query's own row first: its rows fill the list with small values
        const int r = (rq + Rows<D>::v / 2) % Rows<D>::v;
        uint64_t base = 0;
        bool ok = true;
        int rr = r;
#pragma unroll
        for (int ax = D - 1; ax >= 1; --ax) {
            int pw = 1;
            for (int t = 1; t < ax; ++t) pw *= 3;
            const int64_t y = c[ax] + (int64_t)(rr / pw) - 1;
            rr %= pw;
            ok = ok && y >= 0 && y < g.nc[ax];
            base += (uint64_t)(ok ? y : 0) * g.stride[ax];
        }
        if (!ok) continue;
        const uint64_t klo = base + (uint64_t)x0, khi = base + (uint64_t)x1;
        const uint64_t b = klo >> shift;
        if (!PD_OK(b + 1 < ntab, 41, b)) continue;
        const uint32_t e0 = cell_lower_bound<K>(ckey, tab[b], tab[b + 1], klo);
        uint32_t e1 = e0;
        for (; e1 < ncells && (uint64_t)ckey[e1] <= khi; ++e1) {}   // <= 3 cells
        if (e1 == e0) continue;
        // occupied cells adjacent in ckey hold adjacent records: the row is one
        // record run.  Four candidates' loads and sums are issued together (the
        // loads do not wait on the list), then offered in record order.
        uint32_t j = cstart[e0];
        const uint32_t j1 = cstart[e1];
        if (!PD_OK(j <= j1 && j1 <= nrec, 42, j1)) continue;
        for (; j + 4 <= j1; j += 4) {
            double acc4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                double bv[D];
                load_rec<T, D>(Xs, j + u, bv);
                double acc = 0.0;
#pragma unroll
                for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                acc4[u] = acc;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) list.offer(acc4[u]);
        }
        for (; j < j1; ++j) {
            double bv[D];
            load_rec<T, D>(Xs, j, bv);
            double acc = 0.0;
#pragma unroll
            for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
            list.offer(acc);
        }
    }
    out[qi] = list.result();
}

// d > kMaxDim: dense_query_kernel's tiles (queries transposed in LDS, rows
// streamed through a tile every lane reads as a broadcast) with each lane's
// list in LDS next to them.  The axis loop stops at the first partial sum
// above tau: the sum never decreases, so such a pair could not enter the list.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void dense_kdist_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc, uint64_t nc, int TC,
    double thr, int k, double* __restrict__ out, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    double* Bs = reinterpret_cast<double*>(smem);            // [k][QB]
    T* Qs = reinterpret_cast<T*>(Bs + (size_t)k * QB);       // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                             // [TC][d]
    const uint64_t q0 = (uint64_t)blockIdx.x * QB;
    unsigned nf = 0;
    for (int e = tid; e < QB * d; e += QB) {
        const int row = e / d, ax = e % d;
        const uint64_t gi = q0 + (uint64_t)row;
        const T v = gi < m ? Q[gi * (uint64_t)d + ax] : (T)0;
        nf += isfinite((double)v) ? 0u : 1u;
        Qs[(size_t)ax * QB + row] = v;
    }
    if (nf) atomicAdd(bad, (unsigned long long)nf);
    LdsList list;
    list.init(Bs, tid, QB, k, thr);
    for (uint64_t t0 = 0; t0 < nc; t0 += (uint64_t)TC) {
        const int tc = (int)(nc - t0 < (uint64_t)TC ? nc - t0 : (uint64_t)TC);
        __syncthreads();
        for (int e = tid; e < tc * d; e += QB)
            if (PD_OK(t0 * (uint64_t)d + e < nc * (uint64_t)d, 43, t0 * (uint64_t)d + e))
                Cs[e] = Xc[t0 * (uint64_t)d + e];
        __syncthreads();
        for (int c = 0; c < tc; ++c) {
            const T* cr = Cs + (size_t)c * d;
            const double tau = list.tau();
            double acc = 0.0;
            for (int ax = 0; ax < d; ++ax) {
                acc = within_axis<M>(acc, (double)Qs[(size_t)ax * QB + tid], (double)cr[ax]);
                if (acc > tau) break;
            }
            if (acc <= tau) list.offer(acc);
        }
    }
    const uint64_t gi = q0 + (uint64_t)tid;
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
    if (!PD_OK(w < m * (uint64_t)k, 53, w)) return;
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
    __device__ __forceinline__ void init(int k, double thr_) {
        thr = thr_;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            b[s] = s < KT - k ? -INFINITY : INFINITY;
            l[s] = s < KT - k ? INT32_MIN : INT32_MAX;
        }
    }
    __device__ __forceinline__ double tau() const { return thr < b[KT - 1] ? thr : b[KT - 1]; }
    // lab[j]: the candidate's label, read only once acc has passed tau
    __device__ __forceinline__ void offer(double acc, const int32_t* __restrict__ lab, uint32_t j) {
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
    __device__ __forceinline__ void init(double* base, int32_t* lbase, int lane, int lanes, int k_,
                                         double thr_) {
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
    __device__ __forceinline__ void offer(double acc, const int32_t* __restrict__ lab, uint32_t j) {
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

// kdist_kernel's walk (one lane per query, its own row first, each row one
// record run, four candidates' loads and sums in flight, `order` for the
// cell-sorted sweep) over a pair list.  KT > 0: in registers (k <= KT), each
// lane stores its own row.  KT == 0: in dynamic LDS — k * blockDim.x doubles,
// as many int32, a query number per lane — where each lane orders its row and
// the block then stores the rows side by side (C2, k = 10, ids + acc of all
// points: 80.7 -> 75.4 ms against each lane storing its own).  A non-finite
// query and one more than a cell outside the grid keep an empty list: k slots
// of (-1, +inf).
template <typename T, int D, int M, typename K, int KT>
__global__ __launch_bounds__(kBlock) void knn_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxGrid g,
    const T* __restrict__ Xs, const int32_t* __restrict__ lab, uint64_t nrec,
    const K* __restrict__ ckey, const uint32_t* __restrict__ cstart,
    const uint32_t* __restrict__ tab, uint64_t ntab, uint32_t ncells, int shift, double thr, int k,
    int32_t* __restrict__ ids, double* __restrict__ accs, unsigned long long* __restrict__ bad) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr bool kLds = KT == 0;   // its rows leave through a barrier: no lane exits early
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!kLds && i >= m) return;
    bool live = i < m;
    const uint64_t qi = live ? (order ? (uint64_t)order[i] : i) : 0;
    if (!PD_OK(qi < m, 50, qi)) {
        if (!kLds) return;
        live = false;
    }
    double a[D];
    bool fin = live;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        a[j] = live ? (double)Q[qi * D + j] : 0.0;
        fin = fin && isfinite(a[j]);
    }
    if (live && !fin) atomicAdd(bad, 1ull);
    typename std::conditional<(KT > 0), RegPairs<(KT > 0 ? KT : 1)>, LdsPairs>::type list;
    if constexpr (KT > 0) {
        list.init(k, thr);
    } else {
        double* Bs = reinterpret_cast<double*>(smem);
        list.init(Bs, reinterpret_cast<int32_t*>(Bs + (size_t)k * blockDim.x), (int)threadIdx.x,
                  (int)blockDim.x, k, thr);
    }
    int64_t c[D];
    if (fin && cell_of<D>(a, g, c)) {
        const int64_t x0 = c[0] - 1 < 0 ? 0 : c[0] - 1;
        const int64_t x1 = c[0] + 1 >= g.nc[0] ? g.nc[0] - 1 : c[0] + 1;
        for (int rq = 0; rq < Rows<D>::v; ++rq) {
            // the query's own row first: its rows fill the list with small values
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
            const uint64_t b = klo >> shift;
            if (!PD_OK(b + 1 < ntab, 51, b)) continue;
            const uint32_t e0 = cell_lower_bound<K>(ckey, tab[b], tab[b + 1], klo);
            uint32_t e1 = e0;
            for (; e1 < ncells && (uint64_t)ckey[e1] <= khi; ++e1) {}   // <= 3 cells
            if (e1 == e0) continue;
            uint32_t j = cstart[e0];
            const uint32_t j1 = cstart[e1];
            if (!PD_OK(j <= j1 && j1 <= nrec, 52, j1)) continue;   // covers Xs and lab alike
            for (; j + 4 <= j1; j += 4) {
                double acc4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double bv[D];
                    load_rec<T, D>(Xs, j + u, bv);
                    double acc = 0.0;
#pragma unroll
                    for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                    acc4[u] = acc;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) list.offer(acc4[u], lab, j + u);
            }
            for (; j < j1; ++j) {
                double bv[D];
                load_rec<T, D>(Xs, j, bv);
                double acc = 0.0;
#pragma unroll
                for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                list.offer(acc, lab, j);
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
        Qi[tid] = live ? (uint32_t)qi : 0xFFFFFFFFu;   // m < 2^32 - 1
        __syncthreads();
        for (int e = tid; e < lanes * k; e += lanes) {
            const int rl = e / k, t = e - rl * k;
            const uint32_t q = Qi[rl];
            if (q != 0xFFFFFFFFu)
                knn_store(ids, accs, (uint64_t)q, m, k, t, Bs[(size_t)t * lanes + rl],
                          Li[(size_t)t * lanes + rl]);
        }
    } else {
        list.write(ids, accs, qi, m, k);
    }
}

// d > kMaxDim: dense_kdist_kernel's tiles with the rows' labels streamed beside
// them (as dense_radius_kernel's fill) and each lane's pair list in LDS.  The
// axis loop stops at the first partial sum above tau; a sum equal to tau runs
// to the end and is offered, where its label decides.
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
    const uint64_t q0 = (uint64_t)blockIdx.x * QB;
    unsigned nf = 0;
    for (int e = tid; e < QB * d; e += QB) {
        const int qr = e / d, ax = e % d;
        const uint64_t gi = q0 + (uint64_t)qr;
        const T v = gi < m ? Q[gi * (uint64_t)d + ax] : (T)0;
        nf += isfinite((double)v) ? 0u : 1u;
        Qs[(size_t)ax * QB + qr] = v;
    }
    if (nf) atomicAdd(bad, (unsigned long long)nf);
    const uint64_t gi = q0 + (uint64_t)tid;
    const bool live = gi < m;   // the block's tail lanes sweep nothing and write nothing
    LdsPairs list;
    list.init(Bs, Li, tid, QB, k, thr);
    for (uint64_t t0 = 0; t0 < nc; t0 += (uint64_t)TC) {
        const int tc = (int)(nc - t0 < (uint64_t)TC ? nc - t0 : (uint64_t)TC);
        __syncthreads();
        for (int e = tid; e < tc * d; e += QB)
            if (PD_OK(t0 * (uint64_t)d + e < nc * (uint64_t)d, 54, t0 * (uint64_t)d + e))
                Cs[e] = Xc[t0 * (uint64_t)d + e];
        for (int e = tid; e < tc; e += QB)
            if (PD_OK(t0 + e < nc, 55, t0 + e)) Ls[e] = lab[t0 + e];
        __syncthreads();
        if (!live) continue;
        for (int c = 0; c < tc; ++c) {
            const T* cr = Cs + (size_t)c * d;
            const double tau = list.tau();
            double acc = 0.0;
            for (int ax = 0; ax < d; ++ax) {
                acc = within_axis<M>(acc, (double)Qs[(size_t)ax * QB + tid], (double)cr[ax]);
                if (acc > tau) break;
            }
            if (acc <= tau) list.offer(acc, Ls, (uint32_t)c);
        }
    }
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
    uint32_t n;             // hits so far
    int64_t pos, end, lim;  // FILL: stores go to [pos, lim)
    bool ok;
    __device__ __forceinline__ void open(const int64_t* __restrict__ off, uint64_t qi, uint64_t m,
                                         int64_t cap) {
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
    __device__ __forceinline__ void offer(double acc, double thr, const int32_t* __restrict__ lab,
                                          uint32_t j, int32_t* __restrict__ ids,
                                          double* __restrict__ accs) {
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

// d <= 4: kdist_kernel's walk without the list — one lane per query, its own
// row first, each row one contiguous record run, four candidates' loads and
// sums in flight, `order` for the cell-sorted sweep, nothing for a query more
// than a cell outside the grid.  Hits keep the walk's order, which a given
// index and call fix.  tally[0]: non-finite queries; tally[1]: see RadiusRow.
template <typename T, int D, int M, typename K, int FILL>
__global__ __launch_bounds__(kBlock) void radius_kernel(
    const T* __restrict__ Q, uint64_t m, const uint32_t* __restrict__ order, IxGrid g,
    const T* __restrict__ Xs, const int32_t* __restrict__ lab, uint64_t nrec,
    const K* __restrict__ ckey, const uint32_t* __restrict__ cstart,
    const uint32_t* __restrict__ tab, uint64_t ntab, uint32_t ncells, int shift, double thr,
    uint32_t* __restrict__ cnt, const int64_t* __restrict__ off, int32_t* __restrict__ ids,
    double* __restrict__ accs, int64_t cap, unsigned long long* __restrict__ tally) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint64_t qi = order ? (uint64_t)order[i] : i;
    if (!PD_OK(qi < m, 44, qi)) return;
    RadiusRow<FILL> row;
    row.open(off, qi, m, cap);
    double a[D];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        a[j] = (double)Q[qi * D + j];
        fin = fin && isfinite(a[j]);
    }
    if (!fin) atomicAdd(tally, 1ull);
    int64_t c[D];
    if (fin && cell_of<D>(a, g, c)) {
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
            const uint64_t b = klo >> shift;
            if (!PD_OK(b + 1 < ntab, 46, b)) continue;
            const uint32_t e0 = cell_lower_bound<K>(ckey, tab[b], tab[b + 1], klo);
            uint32_t e1 = e0;
            for (; e1 < ncells && (uint64_t)ckey[e1] <= khi; ++e1) {}   // <= 3 cells
            if (e1 == e0) continue;
            uint32_t j = cstart[e0];
            const uint32_t j1 = cstart[e1];
            if (!PD_OK(j <= j1 && j1 <= nrec, 47, j1)) continue;
            for (; j + 4 <= j1; j += 4) {
                double acc4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double bv[D];
                    load_rec<T, D>(Xs, j + u, bv);
                    double acc = 0.0;
#pragma unroll
                    for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                    acc4[u] = acc;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) row.offer(acc4[u], thr, lab, j + u, ids, accs);
            }
            for (; j < j1; ++j) {
                double bv[D];
                load_rec<T, D>(Xs, j, bv);
                double acc = 0.0;
#pragma unroll
                for (int ax = 0; ax < D; ++ax) acc = within_axis<M>(acc, a[ax], bv[ax]);
                row.offer(acc, thr, lab, j, ids, accs);
            }
        }
    }
    row.close(cnt, qi, cap, tally);
}

// d > kMaxDim: dense_query_kernel's tiles (queries transposed in LDS, rows and
// — for a fill — their labels streamed through a tile every lane reads as a
// broadcast).  The axis loop stops at the first partial sum above thr; a pair
// that is accepted ran it to the end, so its accumulator is the full sum.
template <typename T, int M, int FILL>
__global__ __launch_bounds__(kBlock) void dense_radius_kernel(
    const T* __restrict__ Q, uint64_t m, int d, const T* __restrict__ Xc,
    const int32_t* __restrict__ lab, uint64_t nc, int TC, double thr, uint32_t* __restrict__ cnt,
    const int64_t* __restrict__ off, int32_t* __restrict__ ids, double* __restrict__ accs,
    int64_t cap, unsigned long long* __restrict__ tally) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int QB = (int)blockDim.x, tid = (int)threadIdx.x;
    T* Qs = reinterpret_cast<T*>(smem);                                  // [d][QB]
    T* Cs = Qs + (size_t)d * QB;                                         // [TC][d]
    int32_t* Ls = reinterpret_cast<int32_t*>(Cs + (size_t)TC * d);       // [TC]
    const uint64_t q0 = (uint64_t)blockIdx.x * QB;
    unsigned nf = 0;
    for (int e = tid; e < QB * d; e += QB) {
        const int qr = e / d, ax = e % d;
        const uint64_t gi = q0 + (uint64_t)qr;
        const T v = gi < m ? Q[gi * (uint64_t)d + ax] : (T)0;
        nf += isfinite((double)v) ? 0u : 1u;
        Qs[(size_t)ax * QB + qr] = v;
    }
    if (nf) atomicAdd(tally, (unsigned long long)nf);
    const uint64_t gi = q0 + (uint64_t)tid;
    const bool live = gi < m;   // the block's tail lanes sweep a zero row and emit nothing
    RadiusRow<FILL> row;
    row.open(off, live ? gi : 0, m, cap);
    for (uint64_t t0 = 0; t0 < nc; t0 += (uint64_t)TC) {
        const int tc = (int)(nc - t0 < (uint64_t)TC ? nc - t0 : (uint64_t)TC);
        __syncthreads();
        for (int e = tid; e < tc * d; e += QB)
            if (PD_OK(t0 * (uint64_t)d + e < nc * (uint64_t)d, 48, t0 * (uint64_t)d + e))
                Cs[e] = Xc[t0 * (uint64_t)d + e];
        if constexpr (FILL > 0)
            for (int e = tid; e < tc; e += QB)
                if (PD_OK(t0 + e < nc, 49, t0 + e)) Ls[e] = lab[t0 + e];
        __syncthreads();
        if (!live) continue;
        for (int c = 0; c < tc; ++c) {
            const T* cr = Cs + (size_t)c * d;
            double acc = 0.0;
            for (int ax = 0; ax < d; ++ax) {
                acc = within_axis<M>(acc, (double)Qs[(size_t)ax * QB + tid], (double)cr[ax]);
                if (acc > thr) break;
            }
            row.offer(acc, thr, Ls, (uint32_t)c, ids, accs);
        }
    }
    if (live) row.close(cnt, gi, cap, tally);
}

// The fill of an empty index: every segment must be empty.
__global__ __launch_bounds__(kBlock) void radius_empty_kernel(const int64_t* __restrict__ off,
                                                              uint64_t m, int64_t cap,
                                                              unsigned long long* __restrict__ tally) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    RadiusRow<1> row;
    row.open(off, i, m, cap);
    row.close(nullptr, i, cap, tally);
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

template <typename T, int D, int M, typename K>
void query_grid(Index& ix, const T* Q, uint64_t m, int32_t* out, unsigned long long* bad,
                hipStream_t s) {
    const uint32_t* order = query_order<T, D, K>(ix, Q, m, s);
    hipLaunchKernelGGL((query_kernel<T, D, M, K>), dim3(blocks(m)), dim3(kBlock), 0, s, Q, m, order,
                       ix.g, (const T*)ix.Xs, ix.lab, (const K*)ix.ckey, ix.cstart, ix.clab, ix.tab,
                       ix.ncells, ix.shift, ix.eps, ix.eps * ix.eps, ix.slo, ix.shi, out, bad);
    PD_HIP(hipGetLastError());
}

template <typename T, int D, int M>
void query_grid_k(Index& ix, const T* Q, uint64_t m, int32_t* out, unsigned long long* bad,
                  hipStream_t s) {
    if (ix.key_bytes == 4)
        query_grid<T, D, M, uint32_t>(ix, Q, m, out, bad, s);
    else
        query_grid<T, D, M, uint64_t>(ix, Q, m, out, bad, s);
}

template <typename T, int M>
void query_dense(Index& ix, const T* Q, uint64_t m, int32_t* out, unsigned long long* bad,
                 hipStream_t s) {
    // LDS: QB query rows (<= 32 KiB where a block size allows it) + TC core
    // rows and labels, 60 KiB in all
    const size_t row = (size_t)ix.d * sizeof(T);
    int QB = 256;
    while (QB > 64 && (size_t)QB * row > (32u << 10)) QB >>= 1;
    const size_t budget = 60u << 10;
    if ((size_t)QB * row + row + 4 > budget)
        throw Error(-5, "pd_index_query: d too large for the tile kernel's LDS (d * itemsize <= 944)");
    const int TC = (int)std::min<size_t>(64, (budget - (size_t)QB * row) / (row + 4));
    const size_t lds = (size_t)QB * row + (size_t)TC * (row + 4);
    const double thr = M == 0 ? ix.eps * ix.eps : ix.eps;
    hipLaunchKernelGGL((dense_query_kernel<T, M>), dim3((unsigned)((m + QB - 1) / QB)), dim3(QB),
                       lds, s, Q, m, ix.d, (const T*)ix.Xs, ix.lab, ix.nc, TC, thr, out, bad);
    PD_HIP(hipGetLastError());
}

template <typename T, int M>
void query_m(Index& ix, const T* Q, uint64_t m, int32_t* out, unsigned long long* bad,
             hipStream_t s) {
    switch (ix.d) {
        case 1: query_grid_k<T, 1, M>(ix, Q, m, out, bad, s); break;
        case 2: query_grid_k<T, 2, M>(ix, Q, m, out, bad, s); break;
        case 3: query_grid_k<T, 3, M>(ix, Q, m, out, bad, s); break;
        case 4: query_grid_k<T, 4, M>(ix, Q, m, out, bad, s); break;
        default: query_dense<T, M>(ix, Q, m, out, bad, s); break;
    }
}

template <typename T>
void query_t(Index& ix, const T* Q, uint64_t m, int32_t* out, hipStream_t s) {
    Ctx& w = ix.work;
    unsigned long long* bad = w.arena.get<unsigned long long>("q_bad", 1);
    PD_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    if (ix.nc == 0) {
        hipLaunchKernelGGL((finite_kernel<T>), dim3(grid_for((int64_t)(m * ix.d), 1024)),
                           dim3(kBlock), 0, s, Q, m * (uint64_t)ix.d, bad);
        PD_HIP(hipGetLastError());
        PD_HIP(hipMemsetAsync(out, 0xFF, sizeof(int32_t) * m, s));   // -1
    } else if (ix.metric == 0) {
        query_m<T, 0>(ix, Q, m, out, bad, s);
    } else {
        query_m<T, 1>(ix, Q, m, out, bad, s);
    }
    unsigned long long nbad = 0;
    read_u64(w, bad, 1, &nbad, s);
    if (nbad) throw Error(-1, "pd_index_query: a query has a NaN or infinite coordinate");
}

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

// The list tier of a run-time k (DESIGN.md §12 has the resource report behind
// it): registers up to 8, LDS above, with the block sized so that the list of
// a block stays at 32 KiB — 256 lanes up to k = 16, 128 up to 32, 64 up to 64.
template <typename T, int D, int M, typename K, int KT>
void kdist_launch(Index& ix, const T* Q, uint64_t m, const uint32_t* order, int k, int lanes,
                  double thr, double* out, unsigned long long* bad, hipStream_t s) {
    const size_t lds = KT > 0 ? 0 : (size_t)k * lanes * sizeof(double);
    hipLaunchKernelGGL((kdist_kernel<T, D, M, K, KT>), dim3((unsigned)((m + lanes - 1) / lanes)),
                       dim3(lanes), lds, s, Q, m, order, ix.g, (const T*)ix.Xs, ix.nc,
                       (const K*)ix.ckey, ix.cstart, ix.tab, ix.ntab, ix.ncells, ix.shift, thr, k,
                       out, bad);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "kdist_kernel");
}

template <typename T, int D, int M, typename K>
void kdist_grid(Index& ix, const T* Q, uint64_t m, int k, double thr, double* out,
                unsigned long long* bad, hipStream_t s) {
    const uint32_t* order = query_order<T, D, K>(ix, Q, m, s);
    if (k <= 4)
        kdist_launch<T, D, M, K, 4>(ix, Q, m, order, k, kBlock, thr, out, bad, s);
    else if (k <= 8)
        kdist_launch<T, D, M, K, 8>(ix, Q, m, order, k, kBlock, thr, out, bad, s);
    else
        kdist_launch<T, D, M, K, 0>(ix, Q, m, order, k, k <= 16 ? 256 : k <= 32 ? 128 : 64, thr,
                                    out, bad, s);
}

template <typename T, int D, int M>
void kdist_grid_k(Index& ix, const T* Q, uint64_t m, int k, double thr, double* out,
                  unsigned long long* bad, hipStream_t s) {
    if (ix.key_bytes == 4)
        kdist_grid<T, D, M, uint32_t>(ix, Q, m, k, thr, out, bad, s);
    else
        kdist_grid<T, D, M, uint64_t>(ix, Q, m, k, thr, out, bad, s);
}

template <typename T, int M>
void kdist_dense(Index& ix, const T* Q, uint64_t m, int k, double thr, double* out,
                 unsigned long long* bad, hipStream_t s) {
    // LDS per lane: its query row and its k-slot list; per block also TC rows.
    // The row limit is pd_index_query's (64 lanes of rows + one tile row in
    // 60 KiB).  The block shrinks until its lanes' share is <= 48 KiB (never
    // below 64 lanes); what then passes 60 KiB in all (long rows with a large
    // k) asks for up to 144 KiB of the CU's 160 through the function attribute.
    const size_t row = (size_t)ix.d * sizeof(T);
    if ((size_t)64 * row + row + 4 > (60u << 10))
        throw Error(-5, "pd_index_kdist: d too large for the tile kernel's LDS (d * itemsize <= 944)");
    const size_t lane = row + (size_t)k * sizeof(double);
    int QB = 256;
    while (QB > 64 && (size_t)QB * lane > (48u << 10)) QB >>= 1;
    const size_t budget = (size_t)QB * lane + row <= (60u << 10) ? (60u << 10) : (144u << 10);
    const int TC = (int)std::min<size_t>(64, (budget - (size_t)QB * lane) / row);
    const size_t lds = (size_t)QB * lane + (size_t)TC * row;
    if (lds > (64u << 10))
        PD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_kdist_kernel<T, M>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((dense_kdist_kernel<T, M>), dim3((unsigned)((m + QB - 1) / QB)), dim3(QB),
                       lds, s, Q, m, ix.d, (const T*)ix.Xs, ix.nc, TC, thr, k, out, bad);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "dense_kdist_kernel");
}

template <typename T, int M>
void kdist_m(Index& ix, const T* Q, uint64_t m, int k, double* out, unsigned long long* bad,
             hipStream_t s) {
    const double thr = M == 0 ? ix.eps * ix.eps : ix.eps;
    switch (ix.d) {
        case 1: kdist_grid_k<T, 1, M>(ix, Q, m, k, thr, out, bad, s); break;
        case 2: kdist_grid_k<T, 2, M>(ix, Q, m, k, thr, out, bad, s); break;
        case 3: kdist_grid_k<T, 3, M>(ix, Q, m, k, thr, out, bad, s); break;
        case 4: kdist_grid_k<T, 4, M>(ix, Q, m, k, thr, out, bad, s); break;
        default: kdist_dense<T, M>(ix, Q, m, k, thr, out, bad, s); break;
    }
}

template <typename T>
void kdist_t(Index& ix, const T* Q, uint64_t m, int k, double* out, hipStream_t s) {
    Ctx& w = ix.work;
    unsigned long long* bad = w.arena.get<unsigned long long>("q_bad", 1);
    PD_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    if (ix.nc < (uint64_t)k) {   // fewer than k rows in all (also: an empty index)
        hipLaunchKernelGGL((finite_kernel<T>), dim3(grid_for((int64_t)(m * ix.d), 1024)),
                           dim3(kBlock), 0, s, Q, m * (uint64_t)ix.d, bad);
        PD_HIP(hipGetLastError());
        hipLaunchKernelGGL(fill_f64_kernel, dim3(blocks(m)), dim3(kBlock), 0, s, out, m,
                           (double)INFINITY);
        PD_HIP(hipGetLastError());
    } else if (ix.metric == 0) {
        kdist_m<T, 0>(ix, Q, m, k, out, bad, s);
    } else {
        kdist_m<T, 1>(ix, Q, m, k, out, bad, s);
    }
    unsigned long long nbad = 0;
    read_u64(w, bad, 1, &nbad, s);
    if (nbad) throw Error(-1, "pd_index_kdist: a query has a NaN or infinite coordinate");
}

// kdist_launch's tiers at 12 bytes per slot (DESIGN.md §14 has the resource
// report): registers up to 8; LDS above with kdist's block sizes, so a block's
// list is at most 48 KiB (256 lanes x 16, 128 x 32, 64 x 64 slots) and three
// blocks share a CU's 160 KiB: 12, 6 and 3 waves per CU at the top of each tier.
template <typename T, int D, int M, typename K, int KT>
void knn_launch(Index& ix, const T* Q, uint64_t m, const uint32_t* order, int k, int lanes,
                double thr, int32_t* ids, double* acc, unsigned long long* bad, hipStream_t s) {
    // the LDS list: k pairs per lane and, for the write-out, the lane's query number
    const size_t lds =
        KT > 0 ? 0 : (size_t)lanes * (k * (sizeof(double) + sizeof(int32_t)) + sizeof(uint32_t));
    hipLaunchKernelGGL((knn_kernel<T, D, M, K, KT>), dim3((unsigned)((m + lanes - 1) / lanes)),
                       dim3(lanes), lds, s, Q, m, order, ix.g, (const T*)ix.Xs, ix.lab, ix.nc,
                       (const K*)ix.ckey, ix.cstart, ix.tab, ix.ntab, ix.ncells, ix.shift, thr, k,
                       ids, acc, bad);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "knn_kernel");
}

template <typename T, int D, int M, typename K>
void knn_grid(Index& ix, const T* Q, uint64_t m, int k, double thr, int32_t* ids, double* acc,
              unsigned long long* bad, hipStream_t s) {
    const uint32_t* order = query_order<T, D, K>(ix, Q, m, s);
    if (k <= 4)
        knn_launch<T, D, M, K, 4>(ix, Q, m, order, k, kBlock, thr, ids, acc, bad, s);
    else if (k <= 8)
        knn_launch<T, D, M, K, 8>(ix, Q, m, order, k, kBlock, thr, ids, acc, bad, s);
    else
        knn_launch<T, D, M, K, 0>(ix, Q, m, order, k, k <= 16 ? 256 : k <= 32 ? 128 : 64, thr,
                                  ids, acc, bad, s);
}

template <typename T, int D, int M>
void knn_grid_k(Index& ix, const T* Q, uint64_t m, int k, double thr, int32_t* ids, double* acc,
                unsigned long long* bad, hipStream_t s) {
    if (ix.key_bytes == 4)
        knn_grid<T, D, M, uint32_t>(ix, Q, m, k, thr, ids, acc, bad, s);
    else
        knn_grid<T, D, M, uint64_t>(ix, Q, m, k, thr, ids, acc, bad, s);
}

template <typename T, int M>
void knn_dense(Index& ix, const T* Q, uint64_t m, int k, double thr, int32_t* ids, double* acc,
               unsigned long long* bad, hipStream_t s) {
    // kdist_dense's plan with 12 bytes per slot and a label per tile row.  Per
    // lane: its query row and its k pairs; per block also TC rows and labels.
    // The block shrinks until its lanes' share is <= 48 KiB (never below 64
    // lanes); what then passes 60 KiB in all asks for up to 144 KiB through the
    // function attribute (at most 64 * (944 + 768) = 107 KiB of lanes, which
    // leaves 39 tile rows of 948 bytes).
    const size_t row = (size_t)ix.d * sizeof(T);
    if ((size_t)64 * row + row + 4 > (60u << 10))
        throw Error(-5, "pd_index_kneighbors: d too large for the tile kernel's LDS (d * itemsize <= 944)");
    const size_t lane = row + (size_t)k * (sizeof(double) + sizeof(int32_t));
    int QB = 256;
    while (QB > 64 && (size_t)QB * lane > (48u << 10)) QB >>= 1;
    const size_t budget = (size_t)QB * lane + row + 4 <= (60u << 10) ? (60u << 10) : (144u << 10);
    const int TC = (int)std::min<size_t>(64, (budget - (size_t)QB * lane) / (row + 4));
    const size_t lds = (size_t)QB * lane + (size_t)TC * (row + 4);
    if (lds > (64u << 10))
        PD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_knn_kernel<T, M>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((dense_knn_kernel<T, M>), dim3((unsigned)((m + QB - 1) / QB)), dim3(QB),
                       lds, s, Q, m, ix.d, (const T*)ix.Xs, ix.lab, ix.nc, TC, thr, k, ids, acc,
                       bad);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "dense_knn_kernel");
}

template <typename T, int M>
void knn_m(Index& ix, const T* Q, uint64_t m, int k, int32_t* ids, double* acc,
           unsigned long long* bad, hipStream_t s) {
    const double thr = M == 0 ? ix.eps * ix.eps : ix.eps;
    switch (ix.d) {
        case 1: knn_grid_k<T, 1, M>(ix, Q, m, k, thr, ids, acc, bad, s); break;
        case 2: knn_grid_k<T, 2, M>(ix, Q, m, k, thr, ids, acc, bad, s); break;
        case 3: knn_grid_k<T, 3, M>(ix, Q, m, k, thr, ids, acc, bad, s); break;
        case 4: knn_grid_k<T, 4, M>(ix, Q, m, k, thr, ids, acc, bad, s); break;
        default: knn_dense<T, M>(ix, Q, m, k, thr, ids, acc, bad, s); break;
    }
}

// No short cut for an index with fewer than k rows: the walk returns the rows
// there are.  An index without rows has nothing to walk.
template <typename T>
void knn_t(Index& ix, const T* Q, uint64_t m, int k, int32_t* ids, double* acc, hipStream_t s) {
    Ctx& w = ix.work;
    unsigned long long* bad = w.arena.get<unsigned long long>("q_bad", 1);
    PD_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    if (ix.nc == 0) {
        hipLaunchKernelGGL((finite_kernel<T>), dim3(grid_for((int64_t)(m * ix.d), 1024)),
                           dim3(kBlock), 0, s, Q, m * (uint64_t)ix.d, bad);
        PD_HIP(hipGetLastError());
        hipLaunchKernelGGL(knn_empty_kernel, dim3(blocks(m * (uint64_t)k)), dim3(kBlock), 0, s,
                           ids, acc, m * (uint64_t)k);
        PD_HIP(hipGetLastError());
    } else if (ix.metric == 0) {
        knn_m<T, 0>(ix, Q, m, k, ids, acc, bad, s);
    } else {
        knn_m<T, 1>(ix, Q, m, k, ids, acc, bad, s);
    }
    unsigned long long nbad = 0;
    read_u64(w, bad, 1, &nbad, s);
    if (nbad) throw Error(-1, "pd_index_kneighbors: a query has a NaN or infinite coordinate");
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

template <typename T, int D, int M, typename K, int FILL>
void radius_grid(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    const uint32_t* order = query_order<T, D, K>(ix, Q, m, s);
    hipLaunchKernelGGL((radius_kernel<T, D, M, K, FILL>), dim3(blocks(m)), dim3(kBlock), 0, s, Q, m,
                       order, ix.g, (const T*)ix.Xs, ix.lab, ix.nc, (const K*)ix.ckey, ix.cstart,
                       ix.tab, ix.ntab, ix.ncells, ix.shift, rc.thr, rc.cnt, rc.off, rc.ids, rc.acc,
                       rc.cap, rc.tally);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "radius_kernel");
}

template <typename T, int D, int M, int FILL>
void radius_grid_k(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    if (ix.key_bytes == 4)
        radius_grid<T, D, M, uint32_t, FILL>(ix, Q, m, rc, s);
    else
        radius_grid<T, D, M, uint64_t, FILL>(ix, Q, m, rc, s);
}

template <typename T, int M, int FILL>
void radius_dense(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    // pd_index_query's LDS plan: QB query rows + TC rows and labels in 60 KiB
    const size_t row = (size_t)ix.d * sizeof(T);
    int QB = 256;
    while (QB > 64 && (size_t)QB * row > (32u << 10)) QB >>= 1;
    const size_t budget = 60u << 10;
    if ((size_t)QB * row + row + 4 > budget)
        throw Error(-5, "pd_index_radius: d too large for the tile kernel's LDS (d * itemsize <= 944)");
    const int TC = (int)std::min<size_t>(64, (budget - (size_t)QB * row) / (row + 4));
    const size_t lds = (size_t)QB * row + (size_t)TC * (row + 4);
    hipLaunchKernelGGL((dense_radius_kernel<T, M, FILL>), dim3((unsigned)((m + QB - 1) / QB)),
                       dim3(QB), lds, s, Q, m, ix.d, (const T*)ix.Xs, ix.lab, ix.nc, TC, rc.thr,
                       rc.cnt, rc.off, rc.ids, rc.acc, rc.cap, rc.tally);
    PD_HIP(hipGetLastError());
    check_bounds_ix(s, "dense_radius_kernel");
}

template <typename T, int M, int FILL>
void radius_m(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    switch (ix.d) {
        case 1: radius_grid_k<T, 1, M, FILL>(ix, Q, m, rc, s); break;
        case 2: radius_grid_k<T, 2, M, FILL>(ix, Q, m, rc, s); break;
        case 3: radius_grid_k<T, 3, M, FILL>(ix, Q, m, rc, s); break;
        case 4: radius_grid_k<T, 4, M, FILL>(ix, Q, m, rc, s); break;
        default: radius_dense<T, M, FILL>(ix, Q, m, rc, s); break;
    }
}

template <typename T, int FILL>
void radius_f(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    if (ix.metric == 0)
        radius_m<T, 0, FILL>(ix, Q, m, rc, s);
    else
        radius_m<T, 1, FILL>(ix, Q, m, rc, s);
}

// Either pass over a non-empty index; an empty one only checks the queries
// (and, for a fill, that every segment is empty).
template <typename T>
void radius_t(Index& ix, const T* Q, uint64_t m, const RadiusCall& rc, hipStream_t s) {
    if (ix.nc == 0) {
        hipLaunchKernelGGL((finite_kernel<T>), dim3(grid_for((int64_t)(m * ix.d), 1024)),
                           dim3(kBlock), 0, s, Q, m * (uint64_t)ix.d, rc.tally);
        PD_HIP(hipGetLastError());
        if (rc.off) {
            hipLaunchKernelGGL(radius_empty_kernel, dim3(blocks(m)), dim3(kBlock), 0, s, rc.off, m,
                               rc.cap, rc.tally);
            PD_HIP(hipGetLastError());
        }
    } else if (!rc.off) {
        radius_f<T, 0>(ix, Q, m, rc, s);
    } else if (!rc.acc) {
        radius_f<T, 1>(ix, Q, m, rc, s);
    } else {
        radius_f<T, 2>(ix, Q, m, rc, s);
    }
}

double radius_threshold(const Index& ix, int dtype, int64_t m, double radius, const char* who) {
    const std::string w(who);
    if (!(radius > 0) || !std::isfinite(radius))
        throw Error(-1, w + ": radius must be a finite value > 0");
    if (radius > ix.eps)
        throw Error(-1, w + ": radius exceeds the eps the index was built with (its cells cover "
                        "only eps)");
    if (dtype != ix.dtype) throw Error(-1, w + ": the queries' dtype differs from the index's");
    if (m >= 0xFFFFFFFFll) throw Error(-5, w + ": m must be < 2^32 - 1");
    return ix.metric == 0 ? radius * radius : radius;
}

}  // namespace

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
    if (dtype != ix->dtype) throw Error(-1, "pd_index_query: the queries' dtype differs from the index's");
    if (m >= 0xFFFFFFFFll) throw Error(-5, "pd_index_query: m must be < 2^32 - 1");
    if (m == 0) return;
    if (ix->dtype == 0)
        query_t<float>(*ix, (const float*)Q, (uint64_t)m, out, s);
    else
        query_t<double>(*ix, (const double*)Q, (uint64_t)m, out, s);
}

void index_kdist(Index* ix, const void* Q, int dtype, int64_t m, int k, double* out,
                 hipStream_t s) {
    if (k < 1) throw Error(-1, "pd_index_kdist: k must be >= 1");
    if (k > kKdistMaxK) throw Error(-5, "pd_index_kdist: k must be <= PD_KDIST_MAX_K (64)");
    if (dtype != ix->dtype) throw Error(-1, "pd_index_kdist: the queries' dtype differs from the index's");
    if (m >= 0xFFFFFFFFll) throw Error(-5, "pd_index_kdist: m must be < 2^32 - 1");
    if (m == 0) return;
    if (ix->dtype == 0)
        kdist_t<float>(*ix, (const float*)Q, (uint64_t)m, k, out, s);
    else
        kdist_t<double>(*ix, (const double*)Q, (uint64_t)m, k, out, s);
}

void index_kneighbors(Index* ix, const void* Q, int dtype, int64_t m, int k, int32_t* ids,
                      double* acc, hipStream_t s) {
    if (k < 1) throw Error(-1, "pd_index_kneighbors: k must be >= 1");
    if (k > kKdistMaxK) throw Error(-5, "pd_index_kneighbors: k must be <= PD_KDIST_MAX_K (64)");
    if (dtype != ix->dtype)
        throw Error(-1, "pd_index_kneighbors: the queries' dtype differs from the index's");
    if (m >= 0xFFFFFFFFll) throw Error(-5, "pd_index_kneighbors: m must be < 2^32 - 1");
    if (m == 0) return;
    if (ix->dtype == 0)
        knn_t<float>(*ix, (const float*)Q, (uint64_t)m, k, ids, acc, s);
    else
        knn_t<double>(*ix, (const double*)Q, (uint64_t)m, k, ids, acc, s);
}

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
    rc.tally = w.arena.get<unsigned long long>("q_bad", 2);
    PD_HIP(hipMemsetAsync(rc.tally, 0, 2 * sizeof(unsigned long long), s));
    if (ix->nc) {
        rc.cnt = w.arena.get<uint32_t>("r_cnt", um + 1);
        PD_HIP(hipMemsetAsync(rc.cnt + um, 0, sizeof(uint32_t), s));
    }
    if (ix->dtype == 0)
        radius_t<float>(*ix, (const float*)Q, um, rc, s);
    else
        radius_t<double>(*ix, (const double*)Q, um, rc, s);
    if (ix->nc) {
        // 32-bit counts, 64-bit sums: the total passes 2^32 long before n does
        uint64_t* off = reinterpret_cast<uint64_t*>(offsets);
        size_t tb = 0;
        PD_HIP(rocprim::exclusive_scan(nullptr, tb, rc.cnt, off, (uint64_t)0, (size_t)um + 1,
                                       rocprim::plus<uint64_t>(), s));
        void* tmp = w.arena.get<char>("r_scan_tmp", tb);
        PD_HIP(rocprim::exclusive_scan(tmp, tb, rc.cnt, off, (uint64_t)0, (size_t)um + 1,
                                       rocprim::plus<uint64_t>(), s));
    }
    // the non-finite tally and the total in one round trip
    unsigned long long* h = (unsigned long long*)pinned(w, 2 * sizeof(unsigned long long));
    PD_HIP(hipMemcpyAsync(h, rc.tally, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PD_HIP(hipMemcpyAsync(h + 1, offsets + um, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    sync(s);
    if (h[0]) throw Error(-1, "pd_index_radius_count: a query has a NaN or infinite coordinate");
    if (total_host) *total_host = (int64_t)h[1];
}

void index_radius_fill(Index* ix, const void* Q, int dtype, int64_t m, double radius,
                       const int64_t* offsets, int32_t* ids, double* acc, int64_t capacity,
                       hipStream_t s) {
    RadiusCall rc{};
    rc.thr = radius_threshold(*ix, dtype, m, radius, "pd_index_radius_fill");
    if (capacity < 0) throw Error(-1, "pd_index_radius_fill: capacity < 0");
    if (m == 0) return;
    Ctx& w = ix->work;
    rc.off = offsets;
    rc.ids = ids;
    rc.acc = acc;
    rc.cap = capacity;
    rc.tally = w.arena.get<unsigned long long>("q_bad", 2);
    PD_HIP(hipMemsetAsync(rc.tally, 0, 2 * sizeof(unsigned long long), s));
    if (ix->dtype == 0)
        radius_t<float>(*ix, (const float*)Q, (uint64_t)m, rc, s);
    else
        radius_t<double>(*ix, (const double*)Q, (uint64_t)m, rc, s);
    unsigned long long t[2] = {0, 0};
    read_u64(w, rc.tally, 2, t, s);
    if (t[0]) throw Error(-1, "pd_index_radius_fill: a query has a NaN or infinite coordinate");
    if (t[1])
        throw Error(-1, "pd_index_radius_fill: " + std::to_string(t[1]) + " queries' hits do not "
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
