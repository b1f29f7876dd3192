// The KD partition's split tree and the level tables of its device-decided
// BFS: one definition each, shared by the grid train's halo pass (engine.hip)
// and the KD stages (kd.hip), which must agree bit for bit — a point's halo
// owner is the label pd_kd_labels gives it, and the sharded BFS (pd_kdx_*)
// decides on the same tables as the single-device one (pd_kd_build).
#pragma once

#include "common.hpp"

#include <algorithm>
#include <limits>
#include <vector>

namespace pd {

constexpr int kKdMaxLevels = 16;

// ---------------------------------------------------------------- split tree
// Device view of a finished split tree (pd_train_tree, pd_kd_labels): a
// point's label is found by replaying the BFS splits on its coordinates —
// level l, the label's slot: v[axis] >= boundary moves it to the new label
// (the kd_pass split, R:dbscan/partition.py:66-68).
struct KdTree {
    int nl = 0;                  // levels (0: no tree)
    int ntab[kKdMaxLevels], toff[kKdMaxLevels], eoff[kKdMaxLevels];
    int nslot = 0, ne = 0;       // table sizes
    const int32_t* slot;         // concatenated per level: label -> split index in the level (-1)
    const int32_t* ax_new;       // per split: axis, new label
    const double* bound;         // per split: boundary
};

// The walk's bounds sites (1 slot index, 2 split index, 3 axis): a checker
// returns whether the access may go ahead.  engine.hip passes its PD_OK sites
// (PD_CHECK_BOUNDS builds); this one checks nothing and costs nothing.
struct KdNoCheck {
    __device__ __forceinline__ bool operator()(bool, int, uint64_t) const { return true; }
};

// The label of point v.  The three tables are passed apart from the tree so
// that a kernel can hand in its LDS copies.
template <typename T, int D, typename Ok = KdNoCheck>
__device__ __forceinline__ int kd_tree_label(const KdTree& t, const int32_t* slot,
                                             const int32_t* ax_new, const double* bound,
                                             const T (&v)[D], Ok ok = Ok{}) {
    int lab = 0;
    for (int l = 0; l < t.nl; ++l) {
        if (lab >= t.ntab[l]) continue;
        if (!ok(t.toff[l] + lab < t.nslot, 1, t.toff[l] + lab)) continue;
        const int sl = slot[t.toff[l] + lab];
        if (sl < 0) continue;
        const int e = t.eoff[l] + sl;
        if (!ok(e < t.ne, 2, e)) continue;
        const int ax = ax_new[2 * e];
        if (!ok(ax >= 0 && ax < D, 3, ax)) continue;
        T x = v[0];
#pragma unroll
        for (int j = 1; j < D; ++j) x = ax == j ? v[j] : x;
        if ((double)x >= bound[e]) lab = ax_new[2 * e + 1];
    }
    return lab;
}

// Host side, two steps so that the caller provides the memory: the shape
// (levels, table offsets and sizes), then the packed block
//   slot[nslot] | ax_new[2 ne] | (8-byte aligned) bound[ne]
// written to `host` and the tree's pointers set into `dev`, the device
// address the caller copies the block to.  Host arrays in BFS order: sizes[l]
// splits at level l, then per split cur -> newl when v[axis] >= bound.
inline KdTree kd_tree_shape(int n_levels, const int32_t* sizes, const int32_t* cur) {
    if (n_levels > kKdMaxLevels) throw Error(-5, "KD split tree deeper than 16 levels");
    KdTree t;
    t.nl = std::max(n_levels, 0);
    for (int l = 0; l < t.nl; ++l) {
        if (sizes[l] < 0) throw Error(-1, "bad KD split tree");
        int nt = 1;
        for (int k = 0; k < sizes[l]; ++k) nt = std::max(nt, cur[t.ne + k] + 1);
        t.ntab[l] = nt;
        t.toff[l] = t.nslot;
        t.eoff[l] = t.ne;
        t.nslot += nt;
        t.ne += sizes[l];
    }
    return t;
}

inline size_t kd_tree_int_bytes(const KdTree& t) {
    return (sizeof(int32_t) * ((size_t)t.nslot + 2 * (size_t)t.ne) + 7) & ~size_t(7);
}
inline size_t kd_tree_bytes(const KdTree& t) {
    return kd_tree_int_bytes(t) + sizeof(double) * (size_t)t.ne;
}

// Labels in [0, label_limit), axes in [0, d), a label split at most once per
// level; throws Error(-1) otherwise.
inline void kd_tree_fill(KdTree& t, const int32_t* sizes, const int32_t* cur, const int32_t* axis,
                         const double* bound, const int32_t* newl, int d, int label_limit,
                         char* host, const char* dev) {
    int32_t* slot = (int32_t*)host;
    int32_t* ax_new = slot + t.nslot;
    double* bd = (double*)(host + kd_tree_int_bytes(t));
    std::fill(slot, slot + t.nslot, -1);
    for (int l = 0; l < t.nl; ++l)
        for (int k = 0; k < sizes[l]; ++k) {
            const int e = t.eoff[l] + k, L = cur[e];
            if (L < 0 || L >= label_limit || newl[e] < 0 || newl[e] >= label_limit ||
                axis[e] < 0 || axis[e] >= d || slot[t.toff[l] + L] != -1)
                throw Error(-1, "bad KD split tree");
            slot[t.toff[l] + L] = k;
            ax_new[2 * e] = axis[e];
            ax_new[2 * e + 1] = newl[e];
            bd[e] = bound[e];
        }
    t.slot = (const int32_t*)dev;
    t.ax_new = t.slot + t.nslot;
    t.bound = (const double*)(dev + kd_tree_int_bytes(t));
}

// ---------------------------------------------------------------- BFS level tables
// The device-decided BFS (pd_kd_build, pd_kdx_*) keeps per level one block
//   slot_of[ntab] | axis[S] | newlab[S] | (8-byte aligned) bounds[7 S] | boundary[S]
// slot_of and newlab come from the host's schedule; axis, bounds and boundary
// are written by the decision kernels.
struct KdLevel {
    int S, ntab, first;          // splits, label table length, first split's index overall
    int32_t *slot, *axis, *newlab;
    double *bounds, *boundary;
};

struct KdLevels {
    int n_levels = 0, total = 0;
    std::vector<int> sizes, first, ntab;
    std::vector<size_t> off, off_d;

    size_t bytes() const { return off[n_levels]; }

    // Offsets, ntab and first of the schedule: levels of 1..max_tab splits,
    // labels below max_tab (the level kernels stage the tables in LDS).
    void layout(const char* who, int nl, const int32_t* sz, const int32_t* cur,
                const int32_t* newl, int max_tab) {
        n_levels = nl;
        total = 0;
        sizes.assign(sz, sz + nl);
        first.assign(nl, 0);
        ntab.assign(nl, 1);
        off.assign(nl + 1, 0);
        off_d.assign(nl, 0);
        for (int l = 0; l < nl; ++l) {
            const int S = sizes[l];
            if (S < 1 || S > max_tab) throw Error(-5, std::string(who) + ": level too wide");
            first[l] = total;
            for (int k = 0; k < S; ++k) {
                const int L = cur[total + k], N = newl[total + k];
                if (L < 0 || L >= max_tab || N < 0)
                    throw Error(-5, std::string(who) + ": labels beyond the LDS tables");
                ntab[l] = std::max(ntab[l], L + 1);
            }
            const size_t ints = (size_t)ntab[l] + 2 * S;
            off_d[l] = off[l] + ((sizeof(int32_t) * ints + 7) & ~size_t(7));
            off[l + 1] = off_d[l] + sizeof(double) * 8 * S;
            total += S;
        }
    }

    // The host image of the tables (bytes() long): slot_of and newlab filled,
    // the rest zero.
    void fill(char* h, const int32_t* cur, const int32_t* newl) const {
        std::fill(h, h + bytes(), 0);
        for (int l = 0; l < n_levels; ++l) {
            int32_t* slot = (int32_t*)(h + off[l]);
            const int S = sizes[l];
            for (int k = 0; k < ntab[l]; ++k) slot[k] = -1;
            for (int k = 0; k < S; ++k) {
                slot[cur[first[l] + k]] = k;
                slot[ntab[l] + S + k] = newl[first[l] + k];   // newlab after axis
            }
        }
    }

    // Level l's view of the device copy at `tables`.
    KdLevel level(char* tables, int l) const {
        KdLevel v;
        v.S = sizes[l];
        v.ntab = ntab[l];
        v.first = first[l];
        v.slot = (int32_t*)(tables + off[l]);
        v.axis = v.slot + v.ntab;
        v.newlab = v.axis + v.S;
        v.bounds = (double*)(tables + off_d[l]);
        v.boundary = v.bounds + 7 * v.S;
        return v;
    }
};

}  // namespace pd
