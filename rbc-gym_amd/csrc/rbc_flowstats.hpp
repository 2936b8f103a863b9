// rbc_flowstats.hpp -- horizontal statistics of the solver's state on the device (gfx950); included by rbc_api.hip.
//
// Replaces the host route to the numbers the reference's only experiment records after every env-step (Nu and max |u|, |v|, |w|,
// experiments/flowstats/flowstats_ra.py:64-67) and to the row-wise profile pins (tests/profile_pins.py::row_moments_batch):
// fields to the host, numpy there.  DESIGN.md section 3d has the definitions; in short, for env e and level k
//   prof[e][0..5][k] = mean over the level of  b, u^2, v^2, w^2, b w, b^2   (w: face k, the bottom face of cell k; raw staggered values)
//   ext[e][0..4]     = max |u|, max |v|, max |w| (all nz + 1 faces), min b, max b over the env
// every product and sum in float64 (a float32 state is converted first), NaNs propagated the way numpy's mean / max / min do.
//
// Work split BY LEVEL, one pass, every state value loaded once.  A workgroup is four wave64s.
//   WPL = 1 (levels of up to SMALL_LEVEL cells: a 2D row, a small 3D plane): each wave owns one level of one env, a workgroup four
//           consecutive levels; no LDS, no barrier.
//   WPL = 4 (larger planes): the four waves share one level; their partials meet in LDS and are added in wave order.
// The choice reads the grid alone, and an (env, level) pair is computed by the same instructions in the same order whatever the
// batch: the result of an env is bitwise independent of the batch size and of its position in it.
// Which thread adds which value is fixed relative to the level's START (groups of N = 2 / 4 consecutive values, round robin over the
// threads; the n % N values after the last group go to the first threads), never to its address: odd nx * ny puts every second
// level, and every second env, off the 16-byte grid, and the association of the additions must not follow.  Only the load
// instruction does: one 16-byte load per group (double2 / float4) where the level starts on a 16-byte boundary, N loads per group
// where it does not -- chosen per field, b and w (walked together: b w needs both at the same cell) each by its own address.
// Six float64 sums and five extrema live in registers, are
// reduced in the wave by a fixed butterfly (DPP within a row of 16 lanes, ds_swizzle / ds_bpermute across rows) and leave as
// prof[e][m][k] and lev[e][k][0..4], the level's extrema.  flowstats_fold, a second tiny launch, folds lev over the levels in
// level order.  No atomics, no arrival counters, nothing between workgroups.
//
// NaN: v_max_f64 / v_min_f64 drop NaNs, numpy does not.  A sum of squares is NaN exactly when one of its terms is (the terms are
// non-negative, so no inf - inf), hence the level's sums of u^2, v^2, w^2, b^2 tell whether the level's extremum has to be NaN;
// the fold propagates a NaN level explicitly.
//
// Like the ray-caster, the kernels are compiled without packed float32 instructions (target attribute on the device pass; they
// hold no float32 arithmetic at all -- a float32 state is widened by v_cvt_f64_f32 --, so this is a precaution that costs nothing).
// Cross-lane moves use the builtins directly: the header's __shfl_xor is not inlined into a function whose target features differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define RBC_FS_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define RBC_FS_TARGET
#endif

namespace rbcfs {

constexpr int NT = 256, WAVE = 64;
constexpr int SMALL_LEVEL = 1024;         // cells per level up to which one wave owns a level (16 cells per lane)
constexpr int NSUM = 6, NEXT = 5, NACC = NSUM + NEXT;

// where the fields of one env sit in the state buffer, in elements: resident 2D [b | u | w], streaming [b | u | v | w]
struct Layout {
    size_t env_stride, ou, ov, ow;
    int n_h, nz;                          // cells per level (nx * ny), levels
};

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };

__device__ __forceinline__ RBC_FS_TARGET double nan_f64() { return __builtin_nan(""); }

// value of lane (lane ^ M) for M = 1, 2, and of the mirror lane within 8 / 16 lanes for M = 4, 8: after the steps before it every
// lane of a group of M holds the group's sum, so the mirror lane's value IS lane ^ M's.  M = 16: ds_swizzle, M = 32: ds_bpermute.
template <int M>
__device__ __forceinline__ RBC_FS_TARGET int xor_lane(int v, int lane)
{
    if constexpr (M == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);        // quad_perm [1, 0, 3, 2]
    else if constexpr (M == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
    else if constexpr (M == 4) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    else if constexpr (M == 8) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror
    else if constexpr (M == 16) return __builtin_amdgcn_ds_swizzle(v, 0x401F);                   // bit mode: and 0x1f, or 0, xor 0x10
    else return __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, v);
}

template <int M>
__device__ __forceinline__ RBC_FS_TARGET double xor_lane(double x, int lane)
{
    typedef int int2v __attribute__((ext_vector_type(2)));
    int2v p = __builtin_bit_cast(int2v, x);
    p.x = xor_lane<M>((int)p.x, lane);
    p.y = xor_lane<M>((int)p.y, lane);
    return __builtin_bit_cast(double, p);
}

// the registers of one lane: s = sums of b, u^2, v^2, w^2, b w, b^2; x = max |u|, max |v|, max |w|, min b, max b (NaNs dropped)
struct Acc {
    double s[NSUM], x[NEXT], top2;        // top2: sum of squares of w's top faces (last level only)
    __device__ __forceinline__ RBC_FS_TARGET void clear()
    {
#pragma unroll
        for (int m = 0; m < NSUM; ++m) s[m] = 0.0;
        x[0] = x[1] = x[2] = 0.0;
        x[3] = __builtin_inf(); x[4] = -__builtin_inf();
        top2 = 0.0;
    }
    __device__ __forceinline__ RBC_FS_TARGET void speed(int m, double q)   // m = 1: u, 2: v
    {
        s[m] += q * q;
        x[m - 1] = __builtin_fmax(x[m - 1], __builtin_fabs(q));
    }
    __device__ __forceinline__ RBC_FS_TARGET void cell(double b, double w)
    {
        s[0] += b; s[3] += w * w; s[4] += b * w; s[5] += b * b;
        x[2] = __builtin_fmax(x[2], __builtin_fabs(w));
        x[3] = __builtin_fmin(x[3], b); x[4] = __builtin_fmax(x[4], b);
    }
    __device__ __forceinline__ RBC_FS_TARGET void merge(int m, double o)   // slot m of another lane / wave: 0-5 sums, 6-8 max, 9 min, 10 max
    {
        if (m < NSUM) s[m] += o;
        else if (m == NSUM + 3) x[3] = __builtin_fmin(x[3], o);
        else x[m - NSUM] = __builtin_fmax(x[m - NSUM], o);
    }
    __device__ __forceinline__ RBC_FS_TARGET double get(int m) const { return m < NSUM ? s[m] : x[m - NSUM]; }
    template <int M>
    __device__ __forceinline__ RBC_FS_TARGET void butterfly(int lane)
    {
#pragma unroll
        for (int m = 0; m < NACC; ++m) merge(m, xor_lane<M>(get(m), lane));
        top2 += xor_lane<M>(top2, lane);
    }
};

// elements [N i, N i + N) of the level at p: one 16-byte load where the level starts on a 16-byte boundary (ALIGNED), N loads otherwise
template <typename T, bool ALIGNED>
__device__ __forceinline__ RBC_FS_TARGET typename Vec16<T>::type load_group(const T *__restrict__ p, int i)
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
    if constexpr (ALIGNED) return reinterpret_cast<const V *>(p)[i];
    V r;
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = p[(size_t)i * N + j];
    return r;
}

// MODE 0: a cell's b and w; 1, 2: u, v; 3: the top face of w, which counts for max |w| (and its NaN test, top2) only
template <int MODE>
__device__ __forceinline__ RBC_FS_TARGET void visit(Acc &acc, double p, double q)
{
    if constexpr (MODE == 0) acc.cell(p, q);
    else if constexpr (MODE == 3) { acc.top2 += p * p; acc.x[2] = __builtin_fmax(acc.x[2], __builtin_fabs(p)); }
    else acc.speed(MODE, p);
}

// One level of one field (MODE 0: of b at p and w at q, the same cells) into the accumulators, by the `nthr` threads that share the
// level (this one is number t).  WHICH thread adds WHICH value is fixed relative to the level's start: thread t owns the groups
// [N i, N i + N), i = t, t + nthr, ..., and thread j < n % N the j-th value after the last whole group.  Only the load instruction
// depends on where the level lies in memory, so the sums do not: an env's bits are the same at every position in the batch.
template <typename T, int MODE, bool PA, bool QA>
__device__ __forceinline__ RBC_FS_TARGET void sweep_groups(Acc &acc, const T *__restrict__ p, const T *__restrict__ q, int n, int t, int nthr)
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
    const int ngrp = n / N, tail0 = ngrp * N;
#pragma unroll 2
    for (int i = t; i < ngrp; i += nthr) {
        const V a = load_group<T, PA>(p, i);
        V c = a;
        if constexpr (MODE == 0) c = load_group<T, QA>(q, i);
#pragma unroll
        for (int j = 0; j < N; ++j) visit<MODE>(acc, (double)a[j], (double)c[j]);
    }
    if (t < n - tail0) visit<MODE>(acc, (double)p[tail0 + t], MODE == 0 ? (double)q[tail0 + t] : 0.0);
}

template <typename T, int MODE>
__device__ __forceinline__ RBC_FS_TARGET void sweep(Acc &acc, const T *__restrict__ p, const T *__restrict__ q, int n, int t, int nthr)
{
    const bool pa = reinterpret_cast<uintptr_t>(p) % 16 == 0, qa = MODE != 0 || reinterpret_cast<uintptr_t>(q) % 16 == 0;   // wave-uniform
    if (pa && qa) sweep_groups<T, MODE, true, true>(acc, p, q, n, t, nthr);
    else if (pa) sweep_groups<T, MODE, true, false>(acc, p, q, n, t, nthr);
    else if (qa) sweep_groups<T, MODE, false, true>(acc, p, q, n, t, nthr);
    else sweep_groups<T, MODE, false, false>(acc, p, q, n, t, nthr);
}

// B * ceil(nz / 4) workgroups for WPL = 1, B * nz for WPL = 4; 256 threads.  prof: [B][6][nz], lev: [B][nz][5]
template <typename T, bool HAS_V, int WPL>
__global__ __launch_bounds__(NT) RBC_FS_TARGET void flowstats_levels(const Layout L, const T *__restrict__ state, double *__restrict__ prof,
                                                                     double *__restrict__ lev)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int per_env = (WPL == 1) ? (L.nz + NT / WAVE - 1) / (NT / WAVE) : L.nz, env = blockIdx.x / per_env, kb = blockIdx.x - env * per_env;
    const int k = (WPL == 1) ? kb * (NT / WAVE) + wave : kb;
    const int t = (WPL == 1) ? lane : (int)threadIdx.x, nthr = WPL * WAVE;
    if (WPL == 1 && k >= L.nz) return;                    // whole waves leave; this variant has no barrier
    const T *sb = state + (size_t)env * L.env_stride, *b = sb + (size_t)k * L.n_h, *w = sb + L.ow + (size_t)k * L.n_h;

    Acc acc;
    acc.clear();
    sweep<T, 0>(acc, b, w, L.n_h, t, nthr);
    const T *u = sb + L.ou + (size_t)k * L.n_h, *v = sb + L.ov + (size_t)k * L.n_h;
    sweep<T, 1>(acc, u, u, L.n_h, t, nthr);
    if constexpr (HAS_V) sweep<T, 2>(acc, v, v, L.n_h, t, nthr);
    if (k == L.nz - 1) sweep<T, 3>(acc, w + L.n_h, w + L.n_h, L.n_h, t, nthr);     // the top wall's faces count for max |w| only

    acc.butterfly<1>(lane); acc.butterfly<2>(lane); acc.butterfly<4>(lane);
    acc.butterfly<8>(lane); acc.butterfly<16>(lane); acc.butterfly<32>(lane);

    if constexpr (WPL > 1) {
        __shared__ double part[WPL][NACC + 1];
        double mine = acc.top2;                               // lane m carries slot m to LDS (every lane holds the wave's result)
#pragma unroll
        for (int m = 0; m < NACC; ++m)
            if (lane == m) mine = acc.get(m);
        if (lane <= NACC) part[wave][lane] = mine;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (wave != 0) return;
        acc.clear();
#pragma unroll
        for (int q = 0; q < WPL; ++q) {                   // in wave order
#pragma unroll
            for (int m = 0; m < NACC; ++m) acc.merge(m, part[q][m]);
            acc.top2 += part[q][NACC];
        }
    }
    if (lane >= NACC) return;
    // lane m stores slot m: 0-5 the means, 6-10 the level's extrema -- NaN where the level's sum of squares of that field is
    const double rn = (double)L.n_h;
    double out = 0.0;
#pragma unroll
    for (int m = 0; m < NACC; ++m)
        if (lane == m) out = acc.get(m);
    if (lane < NSUM) {
        prof[((size_t)env * NSUM + lane) * L.nz + k] = out / rn;
    } else {
        const double sq = (lane == NSUM) ? acc.s[1] : (lane == NSUM + 1) ? acc.s[2] : (lane == NSUM + 2) ? acc.s[3] + acc.top2 : acc.s[5];
        lev[((size_t)env * L.nz + k) * NEXT + (lane - NSUM)] = (sq != sq) ? nan_f64() : out;
    }
}

// ext[e][j] = fold over the levels, in level order, of lev[e][k][j]; one thread per (env, j)
__global__ __launch_bounds__(WAVE) RBC_FS_TARGET void flowstats_fold(const double *__restrict__ lev, double *__restrict__ ext, int nz, int total)
{
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= total) return;
    const int e = i / NEXT, j = i - e * NEXT;
    const double *p = lev + (size_t)e * nz * NEXT + j;
    double r = p[0];
    for (int k = 1; k < nz; ++k) {
        const double x = p[(size_t)k * NEXT];
        const double m = (j == 3) ? __builtin_fmin(r, x) : __builtin_fmax(r, x);
        r = (x != x || r != r) ? nan_f64() : m;
    }
    ext[i] = r;
}

// both launches on `stream`.  HAS_V = false: the resident 2D layout [b | u | w] (L.ov unused; v^2 and max |v| come out as exact zeros)
template <typename T, bool HAS_V>
inline hipError_t launch_flowstats(const Layout &L, const T *state, int B, double *prof, double *lev, double *ext, hipStream_t stream)
{
    if (L.n_h <= SMALL_LEVEL)
        hipLaunchKernelGGL((flowstats_levels<T, HAS_V, 1>), dim3((unsigned)B * (unsigned)((L.nz + 3) / 4)), dim3(NT), 0, stream, L, state, prof, lev);
    else
        hipLaunchKernelGGL((flowstats_levels<T, HAS_V, 4>), dim3((unsigned)B * (unsigned)L.nz), dim3(NT), 0, stream, L, state, prof, lev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int total = B * NEXT;
    hipLaunchKernelGGL(flowstats_fold, dim3((unsigned)((total + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, lev, ext, L.nz, total);
    return hipGetLastError();
}

}  // namespace rbcfs
