// HDBSCAN from a mutual-reachability forest: the condensed
// tree at a min_cluster_size m, cluster stabilities, the selection (excess of
// mass or leaves), labels and membership probabilities.
//
// The forest's E edges come ascending by (w, u, v): an edge's position is its
// rank, the merge order of the single-linkage dendrogram.  lambda(e) = 1 /
// dist(e), dist = sqrt(w) for euclidean accumulators, IEEE sqrt and division.
// The dendrogram itself is O(n) deep and never built.  HDBSCAN needs only
//   - the maximal subtrees of fewer than m rows (height < m): stage 1, rounds
//     in which two components unite when the lightest edge out of each is the
//     same edge and they hold fewer than m rows together;
//   - the true splits (both sides >= m rows, at most n / m of them): stage 2,
//     an edge between two final components that is the lightest edge out of
//     neither; compacted in rank order;
//   - the tree of the true splits over the blobs the other edges join: stage
//     3, a lock-free union, then Kruskal over the T split edges on the host (at
//     most 2 (n / m) nodes) and a jump table of it;
//   - each row's cluster: stage 4, from its blob's leaf up the jump table to
//     the highest node whose rank is below the rank of the edge the row's
//     small subtree leaves by;
//   - per cluster reductions: stage 5, rows and lambda_max by integer atomics,
//     the stability sum in a fixed association order (rows sorted by (cluster,
//     row), chunks of 256 consecutive terms summed by a pairwise tree, the
//     chunks of a cluster left to right on the host).
// Clusters are numbered leaves first, ascending by smallest row, then the
// clusters that split, ascending by the rank of their split: parent[x] > x.
// The selection runs on the host over that tree; a last device pass writes
// the labels (rank_labels: numbered by smallest member row) and probabilities.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "compact.hpp"
#include "internal.hpp"
#include "uf.hpp"

namespace pd {
namespace {

// Device-side bounds checks, the scheme of engine.hip and assign.hip
// (-DPD_CHECK_BOUNDS=1 builds).  Sites: 50 a row number from an edge; 51 a
// component's entry (minout, csize, hook); 52 an edge rank; 53 a blob or leaf
// entry; 54 a tree node (the jump table, noderank, birth, the reductions); 55 a
// sorted position of the stability sum.
#ifndef PD_CHECK_BOUNDS
#define PD_CHECK_BOUNDS 0
#endif
#if PD_CHECK_BOUNDS
__device__ unsigned long long g_hd_oob[2];   // [0] violations, [1] the first
__device__ __forceinline__ bool pd_hd_ok(bool c, unsigned site, uint64_t idx) {
    if (!c && atomicAdd(&g_hd_oob[0], 1ull) == 0ull)
        g_hd_oob[1] = ((unsigned long long)site << 48) | (idx & 0xFFFFFFFFFFFFull);
    return c;
}
#define PD_OK(cond, site, idx) pd_hd_ok((cond), (site), (uint64_t)(idx))
#else
#define PD_OK(cond, site, idx) true
#endif

void check_bounds_hd(hipStream_t s, const char* who) {
#if PD_CHECK_BOUNDS
    sync(s);
    unsigned long long h[2] = {0, 0};
    PD_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hd_oob), sizeof(h), 0, hipMemcpyDeviceToHost));
    if (h[0]) {
        const unsigned long long z[2] = {0, 0};
        PD_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_hd_oob), z, sizeof(z), 0, hipMemcpyHostToDevice));
        throw Error(-3, std::string(who) + ": " + std::to_string(h[0]) +
                            " out-of-bounds accesses, first at site " + std::to_string(h[1] >> 48) +
                            " index " + std::to_string(h[1] & 0xFFFFFFFFFFFFull));
    }
#else
    (void)s;
    (void)who;
#endif
}

constexpr int kChunk = kBlock;   // terms of the stability sum per pairwise tree

inline unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// 1 / dist: correctly rounded sqrt and division, never the approximate forms
__device__ __forceinline__ double lambda_of(double w, int root) {
    return __ddiv_rn(1.0, root ? __dsqrt_rn(w) : w);
}

// uf_unite that reports a pair already joined (a cycle in a would-be forest).
__device__ __forceinline__ bool unite_checked(uint32_t* par, uint32_t a, uint32_t b) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    while (a != b) {
        if (a > b) {
            uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expected = b;
        if (__hip_atomic_compare_exchange_strong(par + b, &expected, a, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return true;
        b = uf_find(par, expected);
        a = uf_find(par, a);
    }
    return false;
}

// tally slots
enum : int { kBadEnd = 0, kUnsorted, kCycle, kZero, kMerges, kBadCluster, kTally };

__global__ __launch_bounds__(kBlock) void hd_iota_kernel(uint32_t* __restrict__ a,
                                                         uint32_t* __restrict__ b,
                                                         uint32_t* __restrict__ ones, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    a[i] = (uint32_t)i;
    if (b) b[i] = (uint32_t)i;
    if (ones) ones[i] = 1u;
}

// Stage 0: endpoints in [0, n), w ascending (a NaN fails the comparison), w[0] >
// 0, no cycle: every successful union removes one component, so a list with a
// cycle has a union that finds its ends joined, in whatever order they run.
__global__ __launch_bounds__(kBlock) void hd_check_kernel(const int32_t* __restrict__ u,
                                                          const int32_t* __restrict__ v,
                                                          const double* __restrict__ w, uint64_t E,
                                                          uint64_t n, uint32_t* __restrict__ par,
                                                          unsigned long long* __restrict__ tally) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const double we = w[e];
    if (e == 0 ? !(we > 0.0) : !(w[e - 1] <= we)) atomicAdd(tally + (e == 0 ? kZero : kUnsorted), 1ull);
    const int32_t a = u[e], b = v[e];
    if (a < 0 || b < 0 || (uint64_t)a >= n || (uint64_t)b >= n) {
        atomicAdd(tally + kBadEnd, 1ull);
        return;
    }
    if (!unite_checked(par, (uint32_t)a, (uint32_t)b)) atomicAdd(tally + kCycle, 1ull);
}

// Stage 1, step 1: the lightest (lowest rank) edge out of every component.
__global__ __launch_bounds__(kBlock) void hd_minout_kernel(const int32_t* __restrict__ u,
                                                           const int32_t* __restrict__ v,
                                                           uint64_t E, uint64_t n,
                                                           const uint32_t* __restrict__ comp,
                                                           uint32_t* __restrict__ minout) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const uint32_t ru = (uint32_t)u[e], rv = (uint32_t)v[e];
    if (!PD_OK(ru < n && rv < n, 50, e)) return;
    const uint32_t a = comp[ru], b = comp[rv];
    if (a == b || !PD_OK(a < n && b < n, 51, e)) return;
    atomicMin(minout + a, (uint32_t)e);
    atomicMin(minout + b, (uint32_t)e);
}

// Step 2: a reciprocal pair of fewer than m rows unites, the larger root under
// the smaller.  A component is in at most one such pair (its minout is one
// edge), so the pair's lane alone touches the two entries.
__global__ __launch_bounds__(kBlock) void hd_merge_kernel(const int32_t* __restrict__ u,
                                                          const int32_t* __restrict__ v,
                                                          uint64_t E, uint64_t n,
                                                          const uint32_t* __restrict__ comp,
                                                          const uint32_t* __restrict__ minout,
                                                          uint32_t* __restrict__ csize,
                                                          uint32_t* __restrict__ hook, uint32_t m,
                                                          unsigned long long* __restrict__ tally) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const uint32_t ru = (uint32_t)u[e], rv = (uint32_t)v[e];
    if (!PD_OK(ru < n && rv < n, 50, e)) return;
    const uint32_t a = comp[ru], b = comp[rv];
    if (a == b || !PD_OK(a < n && b < n, 51, e)) return;
    if (minout[a] != (uint32_t)e || minout[b] != (uint32_t)e) return;
    const uint32_t sz = csize[a] + csize[b];
    if (sz >= m) return;
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    hook[hi] = lo;
    csize[lo] = sz;
    atomicAdd(tally + kMerges, 1ull);
}

// Step 3: a row's root was a root before the round, so one hop reaches the new one.
__global__ __launch_bounds__(kBlock) void hd_refresh_kernel(uint32_t* __restrict__ comp,
                                                            const uint32_t* __restrict__ hook,
                                                            uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = comp[i];
    if (PD_OK(c < n, 51, i)) comp[i] = hook[c];
}

// Stage 2: an edge between two final components is a true split iff it is the
// lightest edge out of neither (a side it is the lightest out of is a small
// child of the node; any other side holds that component's parent, >= m rows).
struct SplitEdge {
    const int32_t* u;
    const int32_t* v;
    const uint32_t* comp;
    const uint32_t* minout;
    uint64_t n;
    __device__ __forceinline__ bool operator()(uint32_t e) const {
        const uint32_t ru = (uint32_t)u[e], rv = (uint32_t)v[e];
        if (!PD_OK(ru < n && rv < n, 50, e)) return false;
        const uint32_t a = comp[ru], b = comp[rv];
        if (a == b || !PD_OK(a < n && b < n, 51, e)) return false;
        return minout[a] != e && minout[b] != e;
    }
};

// Stage 3: every other edge joins its ends' blobs.
__global__ __launch_bounds__(kBlock) void hd_blob_kernel(SplitEdge split, uint64_t E,
                                                         uint32_t* __restrict__ bpar) {
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E || split((uint32_t)e)) return;
    const uint32_t ru = (uint32_t)split.u[e], rv = (uint32_t)split.v[e];
    if (PD_OK(ru < split.n && rv < split.n, 50, e)) uf_unite(bpar, ru, rv);
}

__global__ __launch_bounds__(kBlock) void hd_blob_flat_kernel(uint32_t* __restrict__ bpar,
                                                              uint64_t n,
                                                              uint32_t* __restrict__ blob,
                                                              uint32_t* __restrict__ bsize) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = uf_find(bpar, (uint32_t)i);
    blob[i] = r;
    if (PD_OK(r < n, 53, i)) atomicAdd(bsize + r, 1u);
}

// A blob of >= m rows is a leaf of the cluster tree (a smaller one is a whole
// component of fewer than m rows: noise).
struct LeafBlob {
    const uint32_t* blob;
    const uint32_t* bsize;
    uint32_t m;
    __device__ __forceinline__ bool operator()(uint32_t i) const {
        return blob[i] == i && bsize[i] >= m;
    }
};

__global__ __launch_bounds__(kBlock) void hd_leafid_kernel(const uint32_t* __restrict__ leaf_rows,
                                                           uint64_t L, uint64_t n,
                                                           uint32_t* __restrict__ leafid) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= L) return;
    const uint32_t r = leaf_rows[j];
    if (PD_OK(r < n, 53, j)) leafid[r] = (uint32_t)j;
}

// The T split edges as pairs of leaves, with their lambda.
__global__ __launch_bounds__(kBlock) void hd_split_edges_kernel(
    const uint32_t* __restrict__ srank, uint64_t T, uint64_t E, uint64_t n,
    const int32_t* __restrict__ u, const int32_t* __restrict__ v, const double* __restrict__ w,
    const uint32_t* __restrict__ blob, const uint32_t* __restrict__ leafid, int root,
    uint32_t* __restrict__ sa, uint32_t* __restrict__ sb, double* __restrict__ slam) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const uint32_t e = srank[t];
    sa[t] = sb[t] = kNone;
    slam[t] = 0.0;
    if (!PD_OK(e < E, 52, t)) return;
    const uint32_t ru = (uint32_t)u[e], rv = (uint32_t)v[e];
    if (!PD_OK(ru < n && rv < n, 50, e)) return;
    const uint32_t bu = blob[ru], bv = blob[rv];
    if (!PD_OK(bu < n && bv < n, 53, e)) return;
    sa[t] = leafid[bu];
    sb[t] = leafid[bv];
    slam[t] = lambda_of(w[e], root);
}

// Stage 4 and the integer reductions of stage 5.  A row p of a leaf blob left
// its cluster by edge f = minout[comp[p]]; its cluster is the highest node on
// the way up from the leaf whose rank is below f (ranks grow upwards; a leaf
// ranks below everything, a top node's jump is itself).
__global__ __launch_bounds__(kBlock) void hd_locate_kernel(
    uint64_t n, uint64_t E, uint32_t C, const uint32_t* __restrict__ comp,
    const uint32_t* __restrict__ minout, const uint32_t* __restrict__ blob,
    const uint32_t* __restrict__ leafid, const int32_t* __restrict__ up, int levels,
    const uint32_t* __restrict__ noderank, const double* __restrict__ w, int root,
    int32_t* __restrict__ point_cluster, double* __restrict__ point_lambda,
    uint32_t* __restrict__ count, unsigned long long* __restrict__ lmax,
    uint32_t* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int32_t pc = -1;
    double pl = 0.0;
    const uint32_t b = blob[i], c = comp[i];
    if (PD_OK(b < n && c < n, 53, i)) {
        uint32_t x = leafid[b];
        const uint32_t f = minout[c];
        if (x != kNone && f != kNone && PD_OK(x < C && f < E, 54, i)) {
            for (int j = levels - 1; j >= 0; --j) {
                const uint32_t y = (uint32_t)up[(uint64_t)j * C + x];
                if (PD_OK(y < C, 54, i) && noderank[y] < f) x = y;
            }
            pc = (int32_t)x;
            pl = lambda_of(w[f], root);
            atomicAdd(count + x, 1u);
            atomicMax(lmax + x, (unsigned long long)__double_as_longlong(pl));
            atomicMin(first + x, (uint32_t)i);
        }
    }
    point_cluster[i] = pc;
    point_lambda[i] = pl;
}

// The leaves renumbered by smallest row; the sort key (noise last) and the row.
__global__ __launch_bounds__(kBlock) void hd_renumber_kernel(uint64_t n, uint32_t C,
                                                             const uint32_t* __restrict__ perm,
                                                             int32_t* __restrict__ point_cluster,
                                                             uint32_t* __restrict__ key,
                                                             uint32_t* __restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t pc = point_cluster[i];
    uint32_t k = C;
    if (pc >= 0 && PD_OK((uint32_t)pc < C, 54, i)) {
        k = perm[pc];
        point_cluster[i] = (int32_t)k;
    }
    key[i] = k;
    val[i] = (uint32_t)i;
}

// Stage 5, the stability sum.  Block b sums chunk b - chunk_start[x] of cluster
// x: the terms lambda_p - birth(x) of up to kChunk consecutive rows of x in
// ascending row order, each rounded on its own, by the pairwise tree (t[i] +
// t[i + 128]), (.. + 64), ... — one fixed association order.
__global__ __launch_bounds__(kBlock) void hd_chunk_sum_kernel(
    uint32_t nchunks, uint32_t C, uint64_t n, const uint32_t* __restrict__ chunk_start,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ val,
    const double* __restrict__ point_lambda, const double* __restrict__ birth,
    double* __restrict__ partial) {
    __shared__ double sh[kChunk];
    const uint32_t b = blockIdx.x;
    if (b >= nchunks) return;
    uint32_t lo = 0, hi = C;   // the last x with chunk_start[x] <= b
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (chunk_start[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t x = lo;
    const uint32_t cnt = seg_start[x + 1] - seg_start[x];
    const uint32_t at = (b - chunk_start[x]) * (uint32_t)kChunk + threadIdx.x;
    double t = 0.0;
    if (at < cnt) {
        const uint64_t pos = (uint64_t)seg_start[x] + at;
        if (PD_OK(pos < n, 55, pos)) {
            const uint32_t p = val[pos];
            if (PD_OK(p < n, 55, pos)) t = __dsub_rn(point_lambda[p], birth[x]);
        }
    }
    sh[threadIdx.x] = t;
    __syncthreads();
#pragma unroll
    for (int s = kChunk / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = __dadd_rn(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[b] = sh[0];
}

// Stage 6: first[S] = the smallest row of the selected cluster S.
__global__ __launch_bounds__(kBlock) void hd_first_kernel(uint64_t n, int64_t C,
                                                          const int32_t* __restrict__ point_cluster,
                                                          const int32_t* __restrict__ target,
                                                          uint32_t* __restrict__ first,
                                                          unsigned long long* __restrict__ tally) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t c = point_cluster[i];
    if (c < -1 || c >= C) {
        atomicAdd(tally + kBadCluster, 1ull);
        return;
    }
    if (c < 0) return;
    const int32_t t = target[c];
    if (t >= 0 && PD_OK(t < C, 54, i)) atomicMin(first + t, (uint32_t)i);
}

__global__ __launch_bounds__(kBlock) void hd_label_key_kernel(
    uint64_t n, int64_t C, const int32_t* __restrict__ point_cluster,
    const double* __restrict__ point_lambda, const int32_t* __restrict__ target,
    const uint32_t* __restrict__ first, const double* __restrict__ lambda_max,
    uint32_t* __restrict__ key, double* __restrict__ prob) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t c = point_cluster[i];
    uint32_t k = kNone;
    double p = 0.0;
    if (c >= 0 && c < C) {
        const int32_t t = target[c];
        if (t >= 0 && PD_OK(t < C, 54, i)) {
            k = first[t];
            const double lm = lambda_max[t], lp = point_lambda[i];
            p = __ddiv_rn(lp < lm ? lp : lm, lm);
        }
    }
    key[i] = k;
    prob[i] = p;
}

void read_tally(Ctx& ctx, const unsigned long long* dev, unsigned long long* out, hipStream_t s) {
    unsigned long long* h = (unsigned long long*)pinned(ctx, sizeof(unsigned long long) * kTally);
    PD_HIP(hipMemcpyAsync(h, dev, sizeof(unsigned long long) * kTally, hipMemcpyDeviceToHost, s));
    sync(s);
    for (int i = 0; i < kTally; ++i) out[i] = h[i];
}

template <typename T>
void to_host(std::vector<T>& dst, const T* dev, size_t count, hipStream_t s) {
    dst.resize(count);
    if (!count) return;
    PD_HIP(hipMemcpyAsync(dst.data(), dev, sizeof(T) * count, hipMemcpyDeviceToHost, s));
    sync(s);
}

template <typename T>
void to_device(T* dev, const std::vector<T>& src, hipStream_t s) {
    if (src.empty()) return;
    PD_HIP(hipMemcpyAsync(dev, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, s));
    sync(s);   // the vector is pageable and may go away
}

struct StageClock {
    double* ms;
    hipStream_t s;
    std::chrono::steady_clock::time_point t0, last;
    StageClock(double* out, hipStream_t st) : ms(out), s(st) {
        if (ms) {
            for (int i = 0; i < 8; ++i) ms[i] = 0.0;
            sync(s);
        }
        t0 = last = std::chrono::steady_clock::now();
    }
    void mark(int slot) {
        if (!ms) return;
        sync(s);
        const auto now = std::chrono::steady_clock::now();
        ms[slot] += std::chrono::duration<double, std::milli>(now - last).count();
        ms[7] = std::chrono::duration<double, std::milli>(now - t0).count();
        last = now;
    }
};

uint32_t find_host(std::vector<uint32_t>& par, uint32_t x) {
    while (par[x] != x) {
        par[x] = par[par[x]];
        x = par[x];
    }
    return x;
}

}  // namespace

void forest_condense(Ctx& ctx, int64_t n_, int64_t E_, const int32_t* u, const int32_t* v,
                     const double* w, int root, int64_t m_, Condensed& o, hipStream_t s) {
    const char* who = "pd_forest_condense";
    o.n_clusters = 0;
    o.rounds = 0;
    const uint64_t n = (uint64_t)n_, E = (uint64_t)E_;
    StageClock clock(o.stage_ms, s);
    if (n == 0) return;
    const dim3 gn(blocks(n)), ge(blocks(E)), bl(kBlock);
    unsigned long long* tally = ctx.arena.get<unsigned long long>("hd_tally", kTally);
    unsigned long long h[kTally];
    PD_HIP(hipMemsetAsync(tally, 0, sizeof(unsigned long long) * kTally, s));
    uint32_t* hook = ctx.arena.get<uint32_t>("hd_hook", n);    // stage 0's forest, then the
                                                               // rounds' hooks, then the blobs'
    uint32_t* comp = ctx.arena.get<uint32_t>("hd_comp", n);
    uint32_t* csize = ctx.arena.get<uint32_t>("hd_csize", n);  // then the blobs' sizes
    uint32_t* minout = ctx.arena.get<uint32_t>("hd_minout", n);
    // ---- stage 0: the list is a sorted forest over the rows, without a zero weight
    if (E) {
        hipLaunchKernelGGL(hd_iota_kernel, gn, bl, 0, s, hook, (uint32_t*)nullptr,
                           (uint32_t*)nullptr, n);
        hipLaunchKernelGGL(hd_check_kernel, ge, bl, 0, s, u, v, w, E, n, hook, tally);
        PD_HIP(hipGetLastError());
        read_tally(ctx, tally, h, s);
        if (h[kBadEnd]) throw Error(-1, std::string(who) + ": an edge's endpoint is not a row number");
        if (h[kUnsorted]) throw Error(-1, std::string(who) + ": the weights are not ascending");
        if (h[kCycle]) throw Error(-1, std::string(who) + ": the edges have a cycle: not a forest");
        if (h[kZero])
            throw Error(-1, std::string(who) +
                                ": the lightest edge has weight 0 (min_samples or more identical "
                                "rows), which makes lambda infinite: deduplicate the rows, or "
                                "train with sample_weight on the distinct ones");
    }
    clock.mark(0);
    PD_HIP(hipMemsetAsync(o.point_cluster, 0xFF, sizeof(int32_t) * n, s));
    PD_HIP(hipMemsetAsync(o.point_lambda, 0, sizeof(double) * n, s));
    if (E == 0 || (uint64_t)m_ > n) {   // no component reaches m rows: all noise
        sync(s);
        clock.mark(5);
        return;
    }
    const uint32_t m = (uint32_t)m_;
    // ---- stage 1: maximal subtrees of fewer than m rows
    hipLaunchKernelGGL(hd_iota_kernel, gn, bl, 0, s, hook, comp, csize, n);
    const char* trace = std::getenv("PD_HDBSCAN_TRACE");
    FILE* tf = trace && *trace ? std::fopen(trace, "a") : nullptr;
    try {
        unsigned long long merged = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            PD_HIP(hipMemsetAsync(minout, 0xFF, sizeof(uint32_t) * n, s));
            hipLaunchKernelGGL(hd_minout_kernel, ge, bl, 0, s, u, v, E, n, comp, minout);
            hipLaunchKernelGGL(hd_merge_kernel, ge, bl, 0, s, u, v, E, n, comp, minout, csize, hook,
                               m, tally);
            hipLaunchKernelGGL(hd_refresh_kernel, gn, bl, 0, s, comp, hook, n);
            PD_HIP(hipGetLastError());
            check_bounds_hd(s, who);
            read_tally(ctx, tally, h, s);   // the round's one host read
            ++o.rounds;
            const unsigned long long got = h[kMerges] - merged;
            merged = h[kMerges];
            if (tf)
                std::fprintf(tf, "{\"round\": %d, \"ms\": %.3f, \"merges\": %llu}\n", o.rounds,
                             std::chrono::duration<double, std::milli>(
                                 std::chrono::steady_clock::now() - t0).count(), got);
            if (got == 0) break;
            if ((uint64_t)o.rounds > (uint64_t)m)
                throw Error(-3, std::string(who) + ": more than m rounds");
        }
    } catch (...) {
        if (tf) std::fclose(tf);
        throw;
    }
    if (tf) std::fclose(tf);
    clock.mark(1);
    // ---- stage 2: the true splits, in rank order
    const SplitEdge split{u, v, comp, minout, n};
    // (at most n / m - 1 of them; the list is sized for whatever the compaction could write)
    uint32_t* srank = ctx.arena.get<uint32_t>("hd_srank", E);
    const uint64_t T = compact_ordered(ctx, "hd_split", E, split, srank, nullptr, s);
    if (T > n / m) throw Error(-3, std::string(who) + ": more true splits than n / m");
    check_bounds_hd(s, who);
    clock.mark(2);
    // ---- stage 3: blobs, leaves, the cluster tree
    uint32_t* bpar = hook;
    uint32_t* bsize = csize;
    uint32_t* blob = ctx.arena.get<uint32_t>("hd_blob", n);
    uint32_t* leafid = ctx.arena.get<uint32_t>("hd_leafid", n);
    uint32_t* leaf_rows = ctx.arena.get<uint32_t>("hd_leaf_rows", n);
    hipLaunchKernelGGL(hd_iota_kernel, gn, bl, 0, s, bpar, (uint32_t*)nullptr, (uint32_t*)nullptr,
                       n);
    PD_HIP(hipMemsetAsync(bsize, 0, sizeof(uint32_t) * n, s));
    PD_HIP(hipMemsetAsync(leafid, 0xFF, sizeof(uint32_t) * n, s));
    hipLaunchKernelGGL(hd_blob_kernel, ge, bl, 0, s, split, E, bpar);
    hipLaunchKernelGGL(hd_blob_flat_kernel, gn, bl, 0, s, bpar, n, blob, bsize);
    PD_HIP(hipGetLastError());
    const uint64_t L = compact_ordered(ctx, "hd_leaf", n, LeafBlob{blob, bsize, m}, leaf_rows,
                                       nullptr, s);
    if (L > n / m) throw Error(-3, std::string(who) + ": more leaf clusters than n / m");
    const uint64_t C = L + T;
    o.n_clusters = (int64_t)C;
    if ((int64_t)C > o.capacity)
        throw Error(-1, std::string(who) + ": capacity " + std::to_string(o.capacity) +
                            " is below the " + std::to_string(C) + " clusters (2 * (n / m) always "
                            "suffices)");
    if (C == 0) {
        sync(s);
        clock.mark(3);
        return;
    }
    uint32_t* sa = ctx.arena.get<uint32_t>("hd_sa", T);
    uint32_t* sb = ctx.arena.get<uint32_t>("hd_sb", T);
    double* slam = ctx.arena.get<double>("hd_slam", T);
    if (L) hipLaunchKernelGGL(hd_leafid_kernel, dim3(blocks(L)), bl, 0, s, leaf_rows, L, n, leafid);
    if (T)
        hipLaunchKernelGGL(hd_split_edges_kernel, dim3(blocks(T)), bl, 0, s, srank, T, E, n, u, v, w,
                           blob, leafid, root, sa, sb, slam);
    PD_HIP(hipGetLastError());
    check_bounds_hd(s, who);
    std::vector<uint32_t> h_rank, h_sa, h_sb;
    std::vector<double> h_slam;
    to_host(h_rank, srank, T, s);
    to_host(h_sa, sa, T, s);
    to_host(h_sb, sb, T, s);
    to_host(h_slam, slam, T, s);
    clock.mark(3);
    // Kruskal over the T split edges: node L + t is the split of rank h_rank[t]
    std::vector<int32_t> parent(C, -1);
    std::vector<uint32_t> noderank(C, 0);
    std::vector<uint8_t> is_split(C, 0);
    {
        std::vector<uint32_t> lpar(L), top(L);
        std::iota(lpar.begin(), lpar.end(), 0u);
        std::iota(top.begin(), top.end(), 0u);
        for (uint64_t t = 0; t < T; ++t) {
            if (h_sa[t] >= L || h_sb[t] >= L)
                throw Error(-3, std::string(who) + ": a true split touches a blob of fewer than m rows");
            const uint32_t ra = find_host(lpar, h_sa[t]), rb = find_host(lpar, h_sb[t]);
            if (ra == rb) throw Error(-1, std::string(who) + ": the edges have a cycle: not a forest");
            const uint32_t x = (uint32_t)(L + t);
            parent[top[ra]] = parent[top[rb]] = (int32_t)x;
            noderank[x] = h_rank[t];
            is_split[x] = 1;
            const uint32_t lo = std::min(ra, rb), hi = std::max(ra, rb);
            lpar[hi] = lo;
            top[lo] = x;
        }
    }
    // depth, birth, the jump table (a parent's number is above its children's)
    std::vector<double> birth(C, 0.0);
    int levels = 1;
    {
        std::vector<uint32_t> depth(C, 0);
        uint32_t deepest = 0;
        for (uint64_t x = C; x-- > 0;)
            if (parent[x] >= 0) {
                depth[x] = depth[parent[x]] + 1;
                deepest = std::max(deepest, depth[x]);
                birth[x] = h_slam[(uint64_t)parent[x] - L];
            }
        while ((1ull << levels) <= deepest) ++levels;
    }
    std::vector<int32_t> up((size_t)levels * C);
    for (uint64_t x = 0; x < C; ++x) up[x] = parent[x] >= 0 ? parent[x] : (int32_t)x;
    for (int j = 1; j < levels; ++j)
        for (uint64_t x = 0; x < C; ++x)
            up[(size_t)j * C + x] = up[(size_t)(j - 1) * C + up[(size_t)(j - 1) * C + x]];
    int32_t* d_up = ctx.arena.get<int32_t>("hd_up", up.size());
    uint32_t* d_noderank = ctx.arena.get<uint32_t>("hd_noderank", C);
    double* d_birth = ctx.arena.get<double>("hd_birth", C);
    to_device(d_up, up, s);
    to_device(d_noderank, noderank, s);
    clock.mark(4);
    // ---- stage 4 (+ rows, lambda_max and smallest row per cluster)
    uint32_t* count = ctx.arena.get<uint32_t>("hd_count", C);
    uint32_t* first = ctx.arena.get<uint32_t>("hd_first", C);
    unsigned long long* lmax = ctx.arena.get<unsigned long long>("hd_lmax", C);
    PD_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t) * C, s));
    PD_HIP(hipMemsetAsync(first, 0xFF, sizeof(uint32_t) * C, s));
    PD_HIP(hipMemsetAsync(lmax, 0, sizeof(unsigned long long) * C, s));
    hipLaunchKernelGGL(hd_locate_kernel, gn, bl, 0, s, n, E, (uint32_t)C, comp, minout, blob, leafid,
                       d_up, levels, d_noderank, w, root, o.point_cluster, o.point_lambda, count,
                       lmax, first);
    PD_HIP(hipGetLastError());
    check_bounds_hd(s, who);
    std::vector<uint32_t> h_count, h_first;
    std::vector<unsigned long long> h_lmax;
    to_host(h_count, count, C, s);
    to_host(h_first, first, C, s);
    to_host(h_lmax, lmax, C, s);
    clock.mark(5);
    // ---- stage 5: the leaves by smallest row, then the per-cluster results
    std::vector<uint32_t> perm(C);
    std::iota(perm.begin(), perm.end(), 0u);
    {
        std::vector<uint32_t> by_first(L);
        std::iota(by_first.begin(), by_first.end(), 0u);
        std::sort(by_first.begin(), by_first.end(),
                  [&](uint32_t a, uint32_t b) { return h_first[a] < h_first[b]; });
        for (uint64_t j = 0; j < L; ++j) perm[by_first[j]] = (uint32_t)j;
    }
    std::vector<int64_t> own(C), below(C);
    for (uint64_t x = 0; x < C; ++x) {
        const uint32_t y = perm[x];
        o.parent[y] = parent[x];   // a split node keeps its number
        o.birth[y] = birth[x];
        own[y] = h_count[x];
        double lm;
        std::memcpy(&lm, &h_lmax[x], sizeof(double));
        if (is_split[x]) lm = std::max(lm, h_slam[x - L]);
        o.lambda_max[y] = lm;
        o.death[y] = is_split[x] ? h_slam[x - L] : lm;
    }
    for (uint64_t y = 0; y < C; ++y) birth[y] = o.birth[y];
    below = own;
    for (uint64_t y = 0; y < C; ++y)
        if (o.parent[y] >= 0) below[o.parent[y]] += below[y];
    std::vector<uint32_t> seg(C + 1, 0), chunk(C + 1, 0);
    for (uint64_t y = 0; y < C; ++y) {
        o.size[y] = below[y];
        seg[y + 1] = seg[y] + (uint32_t)own[y];
        chunk[y + 1] = chunk[y] + (uint32_t)((own[y] + kChunk - 1) / kChunk);
    }
    const uint32_t nchunks = chunk[C];
    uint32_t* d_perm = ctx.arena.get<uint32_t>("hd_perm", C);
    uint32_t* d_seg = ctx.arena.get<uint32_t>("hd_seg", C + 1);
    uint32_t* d_chunk = ctx.arena.get<uint32_t>("hd_chunk", C + 1);
    double* partial = ctx.arena.get<double>("hd_partial", nchunks);
    uint32_t* key = ctx.arena.get<uint32_t>("hd_key", n);
    uint32_t* val = ctx.arena.get<uint32_t>("hd_val", n);
    to_device(d_perm, perm, s);
    to_device(d_seg, seg, s);
    to_device(d_chunk, chunk, s);
    to_device(d_birth, birth, s);
    hipLaunchKernelGGL(hd_renumber_kernel, gn, bl, 0, s, n, (uint32_t)C, d_perm, o.point_cluster,
                       key, val);
    PD_HIP(hipGetLastError());
    int nb = 1;
    while (nb < 32 && (C >> nb)) ++nb;
    sort_pairs_inplace(ctx, key, 4, val, n, nb, s);
    std::vector<double> h_partial;
    if (nchunks) {
        hipLaunchKernelGGL(hd_chunk_sum_kernel, dim3(nchunks), bl, 0, s, nchunks, (uint32_t)C, n,
                           d_chunk, d_seg, val, o.point_lambda, d_birth, partial);
        PD_HIP(hipGetLastError());
    }
    check_bounds_hd(s, who);
    to_host(h_partial, partial, nchunks, s);
    for (uint64_t y = 0; y < C; ++y) {
        double st = 0.0;
        for (uint32_t c = chunk[y]; c < chunk[y + 1]; ++c) st += h_partial[c];
        if (y >= L) st += (double)(below[y] - own[y]) * (o.death[y] - o.birth[y]);
        o.stability[y] = st;
    }
    sync(s);
    clock.mark(6);
}

void condensed_select(int64_t C, const int32_t* parent, const double* stability, int method,
                      int allow_single, int32_t* target) {
    const char* who = "pd_condensed_select";
    if (method != 0 && method != 1)
        throw Error(-1, std::string(who) + ": method must be 0 (eom) or 1 (leaf)");
    int64_t tops = 0;
    for (int64_t x = 0; x < C; ++x) {
        if (parent[x] == -1)
            ++tops;
        else if (parent[x] <= x || parent[x] >= C)
            throw Error(-1, std::string(who) + ": parent[x] must be -1 or in (x, n_clusters)");
        if (!(stability[x] >= 0.0))
            throw Error(-1, std::string(who) + ": a stability is negative or NaN");
    }
    const bool sole = tops == 1;
    std::vector<double> childsum(C, 0.0);
    std::vector<uint8_t> has_child(C, 0), sel(C, 0);
    for (int64_t x = 0; x < C; ++x) {   // children before parents
        const int32_t p = parent[x];
        const bool ok = !(sole && p < 0 && !allow_single);
        double best = stability[x];
        if (!has_child[x])
            sel[x] = ok;
        else if (method == 0 && ok && stability[x] >= childsum[x])
            sel[x] = 1;
        else
            best = childsum[x];
        if (p >= 0) {
            childsum[p] += best;
            has_child[p] = 1;
        }
    }
    for (int64_t x = C; x-- > 0;) {     // parents before children
        const int32_t p = parent[x];
        target[x] = (p >= 0 && target[p] >= 0) ? target[p] : (sel[x] ? (int32_t)x : -1);
    }
}

int64_t condensed_labels(Ctx& ctx, int64_t n_, int64_t C, const int32_t* point_cluster,
                         const double* point_lambda, const int32_t* target_host,
                         const double* lambda_max_host, int32_t* labels, double* prob,
                         hipStream_t s) {
    const char* who = "pd_condensed_labels";
    if (n_ == 0) return 0;
    const uint64_t n = (uint64_t)n_;
    for (int64_t x = 0; x < C; ++x) {
        if (target_host[x] < -1 || target_host[x] >= C)
            throw Error(-1, std::string(who) + ": target[x] must be -1 or a cluster number");
        if (target_host[x] >= 0 && !(lambda_max_host[target_host[x]] > 0.0))
            throw Error(-1, std::string(who) + ": lambda_max of a selected cluster must be > 0");
    }
    const dim3 gn(blocks(n)), bl(kBlock);
    unsigned long long* tally = ctx.arena.get<unsigned long long>("hd_tally", kTally);
    PD_HIP(hipMemsetAsync(tally, 0, sizeof(unsigned long long) * kTally, s));
    int32_t* d_target = ctx.arena.get<int32_t>("hd_target", (size_t)C);
    double* d_lmax = ctx.arena.get<double>("hd_sel_lmax", (size_t)C);
    uint32_t* first = ctx.arena.get<uint32_t>("hd_first", (size_t)C);
    uint32_t* key = ctx.arena.get<uint32_t>("hd_key", n);
    if (C) {
        PD_HIP(hipMemcpyAsync(d_target, target_host, sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
        PD_HIP(hipMemcpyAsync(d_lmax, lambda_max_host, sizeof(double) * C, hipMemcpyHostToDevice, s));
        PD_HIP(hipMemsetAsync(first, 0xFF, sizeof(uint32_t) * C, s));
    }
    hipLaunchKernelGGL(hd_first_kernel, gn, bl, 0, s, n, C, point_cluster, d_target, first, tally);
    hipLaunchKernelGGL(hd_label_key_kernel, gn, bl, 0, s, n, C, point_cluster, point_lambda,
                       d_target, first, d_lmax, key, prob);
    PD_HIP(hipGetLastError());
    rank_labels_async(ctx, key, n, labels, s);
    const int64_t ncl = rank_labels_count(ctx, s);   // syncs: the host arrays were read
    check_bounds_hd(s, who);
    unsigned long long h[kTally];
    read_tally(ctx, tally, h, s);
    if (h[kBadCluster])
        throw Error(-1, std::string(who) + ": a point_cluster entry is no cluster number");
    return ncl;
}

}  // namespace pd
