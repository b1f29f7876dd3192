// The neighbour predicate and the sorted-record loads, shared by the train's
// sweeps (engine.hip) and the assignment index (assign.hip).
//
// Exactness: the predicate is sklearn's kd_tree leaf test
// (SK:neighbors/_binary_tree.pxi.tp:1951-1955, SK:metrics/_dist_metrics.pxd.tp:
// 39-49): fp64, per-axis difference, squared and summed in axis order with
// every product and sum rounded separately (__dmul_rn/__dadd_rn: no FMA), then
// `<= eps*eps`.  Inputs (fp32 or fp64) are widened exactly.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace pd {
namespace {

// Sorted-record layout: 3-D records are padded to 4 components so one
// 16-byte (fp32) load fetches a candidate; other D are packed.
template <int D>
struct Stride {
    static constexpr int v = (D == 3) ? 4 : D;
};

template <typename T, int D>
__device__ __forceinline__ void load_rec(const T* __restrict__ Xs, uint32_t j, double (&v)[D]) {
    constexpr int S = Stride<D>::v;
    if constexpr (std::is_same<T, float>::value && S == 4) {
        const float4 f = *reinterpret_cast<const float4*>(Xs + (uint64_t)j * 4);
        v[0] = f.x;
        v[1] = f.y;
        v[2] = f.z;
        if constexpr (D == 4) v[3] = f.w;
    } else if constexpr (std::is_same<T, float>::value && S == 2) {
        const float2 f = *reinterpret_cast<const float2*>(Xs + (uint64_t)j * 2);
        v[0] = f.x;
        v[1] = f.y;
    } else if constexpr (std::is_same<T, double>::value && S >= 2) {
        const double2* p = reinterpret_cast<const double2*>(Xs + (uint64_t)j * S);
        const double2 u = p[0];
        v[0] = u.x;
        v[1] = u.y;
        if constexpr (S == 4) {
            const double2 w = p[1];
            v[2] = w.x;
            if constexpr (D == 4) v[3] = w.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = (double)Xs[(uint64_t)j * S + k];
    }
}

// sklearn kd_tree leaf predicate, exact: fp64, axis order, every product and
// sum rounded separately (no FMA), `<= eps*eps` (cityblock: `<= eps`).
template <int D, int M>
__device__ __forceinline__ bool within(const double (&a)[D], const double (&b)[D], double eps,
                                       double eps2) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const double t = __dadd_rn(a[j], -b[j]);
        if constexpr (M == 0)
            acc = __dadd_rn(acc, __dmul_rn(t, t));
        else
            acc = __dadd_rn(acc, fabs(t));
    }
    return M == 0 ? (acc <= eps2) : (acc <= eps);
}

// Raw candidate load (input precision).
template <typename T, int D>
__device__ __forceinline__ void load_raw(const T* __restrict__ Xs, uint32_t j, T (&v)[D]) {
    constexpr int S = Stride<D>::v;
    if constexpr (std::is_same<T, float>::value && S == 4) {
        const float4 f = *reinterpret_cast<const float4*>(Xs + (uint64_t)j * 4);
        v[0] = f.x;
        v[1] = f.y;
        v[2] = f.z;
        if constexpr (D == 4) v[3] = f.w;
    } else if constexpr (std::is_same<T, float>::value && S == 2) {
        const float2 f = *reinterpret_cast<const float2*>(Xs + (uint64_t)j * 2);
        v[0] = f.x;
        v[1] = f.y;
    } else if constexpr (std::is_same<T, double>::value && S >= 2) {
        const double2* p = reinterpret_cast<const double2*>(Xs + (uint64_t)j * S);
        const double2 u = p[0];
        v[0] = u.x;
        v[1] = u.y;
        if constexpr (S == 4) {
            const double2 w = p[1];
            v[2] = w.x;
            if constexpr (D == 4) v[3] = w.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = Xs[(uint64_t)j * S + k];
    }
}

// The neighbour predicate as the sweeps use it.  fp32 inputs are screened
// in fp32 first: with every coordinate an fp32 value, the fp32 distance has
// relative error <= (D+2)*2^-24 < 2^-18, so a result below eps^2*(1-2^-18)
// (rounded down to fp32) or above eps^2*(1+2^-18) (rounded up) already
// decides the exact fp64 test; only pairs inside that band (ties) run it.
// fp64 inputs always take the exact path.
template <typename T, int D, int M>
struct Pred {
    double a[D];
    T ar[D];
    double eps, eps2;
    float lo, hi;
    __device__ __forceinline__ bool operator()(const T (&b)[D]) const {
        if constexpr (std::is_same<T, float>::value) {
            float d = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float t = ar[j] - b[j];
                if constexpr (M == 0)
                    d = __builtin_fmaf(t, t, d);
                else
                    d += fabsf(t);
            }
            if (d <= lo) return true;
            if (!(d <= hi)) return false;
        }
        double bb[D];
#pragma unroll
        for (int j = 0; j < D; ++j) bb[j] = (double)b[j];
        return within<D, M>(a, bb, eps, eps2);
    }
    // Branch-free screen: in = decided inside, maybe = needs exact(); fp64
    // inputs are always "maybe".
    __device__ __forceinline__ void screen(const T (&b)[D], bool& in, bool& maybe) const {
        if constexpr (std::is_same<T, float>::value) {
            float d = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float t = ar[j] - b[j];
                if constexpr (M == 0)
                    d = __builtin_fmaf(t, t, d);
                else
                    d += fabsf(t);
            }
            in = d <= lo;
            maybe = !in & (d <= hi);
        } else {
            in = false;
            maybe = true;
        }
    }
    __device__ __forceinline__ bool exact(const T (&b)[D]) const {
        double bb[D];
#pragma unroll
        for (int j = 0; j < D; ++j) bb[j] = (double)b[j];
        return within<D, M>(a, bb, eps, eps2);
    }
};

template <typename T, int D, int M>
__device__ __forceinline__ Pred<T, D, M> make_pred(const T* __restrict__ Xs, uint32_t r,
                                                   const double (&a)[D], double eps, double eps2,
                                                   float lo, float hi) {
    Pred<T, D, M> p;
#pragma unroll
    for (int j = 0; j < D; ++j) p.a[j] = a[j];
    load_raw<T, D>(Xs, r, p.ar);
    p.eps = eps;
    p.eps2 = eps2;
    p.lo = lo;
    p.hi = hi;
    return p;
}

// One axis of `within` for callers whose dimension is a run-time value (the
// d > 4 assignment tiles): the same difference, product and sum, each rounded
// on its own, so a loop of these over the axes in order equals within<D, M>.
// Every term is >= 0, so acc never decreases and a caller may stop at the
// first acc above the threshold.
template <int M>
__device__ __forceinline__ double within_axis(double acc, double a, double b) {
    const double t = __dadd_rn(a, -b);
    if constexpr (M == 0)
        return __dadd_rn(acc, __dmul_rn(t, t));
    else
        return __dadd_rn(acc, fabs(t));
}

}  // namespace
}  // namespace pd
