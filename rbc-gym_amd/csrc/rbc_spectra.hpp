// rbc_spectra.hpp -- horizontal power and co-spectra of the solver's state on the device (gfx950); included by rbc_api.hip.
//
// Replaces the host route to every spectral diagnostic of the project (fields to the host, numpy.fft.rfft there: the moduli and
// cross phases of tests/spectral_invariants.py, the "k = 2 power" columns of VERDICT.md) and gives the 3D envs the one they lack.
// DESIGN.md section 3e has the definitions; in short, with F_j[m] = (1/nx) sum_i f[j][i] e^{-2 pi i m i / nx} the transform of row j
// of level k (raw staggered values: cell level k of b, u, v, face k of w) and c_m the one-sided weight (1 for m = 0 and the Nyquist
// mode of an even nx, 2 otherwise),
//   px[e][0..3][k][m] = c_m mean_j |F_j[m]|^2 for f = b, u, v, w       px[e][4 | 5][k][m] = c_m mean_j Re | Im (B_j[m] conj W_j[m])
// and py the same along y with the mean over x (3D handles).  Float64 throughout, a float32 state is widened as it is staged.
//
// TWO REAL FIELDS PER COMPLEX TRANSFORM.  A staged line is Z = b + i w, a second one u + i v (u + 0 i on a 2D handle).  With
// P = Z[m] and Q = conj Z[(n - m) mod n]:  B = (P + Q) / 2,  W = (P - Q) / (2 i); one pass over (P, Q) yields |B|^2, |W|^2 and both
// parts of B conj W.  Four real fields, six outputs, two complex transforms per row.  The transforms are the float64 slab_fft<N1>
// (n = 8 * {4, 6, 8, 12}, a whole small DFT in registers; see fast_n1) and slab_dft (every other n, odd and prime included) of the pressure
// solve, inlined at the call so that they are compiled under this file's target attribute; lanes run along LINES in both.
//
// spectra_x: one workgroup of 256 threads owns one (env, level) and loops over blocks of R rows (ny > 1), or owns a run of R
//   consecutive levels, one row each (2D handles).  Per block: coalesced loads of the R rows of the four fields (a block of rows is
//   one contiguous run of R * nx values per field) into 2 R LDS lines of pitch nx | 1 complex values -- odd in units of 16 bytes, so
//   the lanes of an LDS access, which sit on consecutive lines at the same element, fall on different bank quads --, ONE transform
//   of all 2 R lines, then the (P, Q) pass with lanes along m (consecutive 16-byte values of one line: conflict-free).
// spectra_y (3D): one workgroup per (env, level) loops over blocks of TX columns.  Rows of TX values are staged with loads
//   coalesced along x into lines that run along y: element stride = the pitch 2 TX, line stride 1.  Consecutive lanes of the
//   transform and of the (P, Q) pass (lanes along columns there) touch consecutive 16-byte values, which a ds_read_b64 / b128
//   serves without a bank conflict whatever the pitch is.
// Sums over rows (columns) live in LDS entries owned by ONE thread each: thread (g, m) adds the rows g, g + G, ... of every block in
// ascending order; the G partials of a mode are added in the order g = 0 .. G - 1 at the end, scaled once by c_m / (n^2 n_other)
// and stored once.  R, TX and G follow from the grid alone (plan_x / plan_y, at most about 64 KB of LDS: two workgroups per CU), which
// thread adds which value from the row and column numbers alone -- never from an address: an (env, level) is computed by the same
// instructions in the same order whatever the batch, the env's position in it or the alignment of its planes.
// No atomics, no arrival counters, nothing between workgroups; every loop is bounded by the grid.
//
// A ZERO PARTNER.  Unpacking leaves in G a rounding residue of F (~2^-53 |F|) where g is identically zero -- w on face 0, the wall, at
// every level 0; v of a 2D handle -- and the power of a zero field must be zero, not 1e-32.  Staging notes per line and part whether any
// value differs from 0 (a NaN does); where none does, that part's transform is 0 times its partner's: exactly zero, or NaN with it.
//
// NaN: a NaN anywhere in a line reaches every mode of its transform (every output is a sum over all inputs), so b and w turn NaN
// together and u and v do: channels 0, 3, 4, 5 of the level, or 1 and 2 (2D handles: 1 only; channel 2 is written as 0, not computed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rbc3d_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define RBC_SP_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define RBC_SP_TARGET
#endif

namespace rbcsp {

using cplx = rbc3::real2;                  // two doubles, 16 bytes
constexpr int NT = 256, NCH = 6;
constexpr size_t LDS_TARGET = 64 * 1024, LDS_CEILING = 160 * 1024;

// where the fields of one env sit in the state buffer, in elements: resident 2D [b | u | w], streaming [b | u | v | w]
struct Layout {
    size_t env_stride, ou, ov, ow;
    int nx, ny, nz;
};

// transformed length n = n1 * n2 (factor2), lines per block (R rows / levels, or TX columns), thread groups G that share a mode
struct Plan {
    int n1, n2, blk, G;
    size_t lds;
};

inline int line_pitch(int n) { return n | 1; }

// LDS of spectra_x: 2 R lines staged + as many for the transform, nx twiddles, the G * 6 * (nx/2 + 1) sums
// (+ the lines' non-zero marks: two parts of 2 R lines, one set per block parity)
inline size_t lds_x(int nx, int R, int G) { return ((size_t)4 * R * line_pitch(nx) + nx) * sizeof(cplx) + (size_t)G * NCH * (nx / 2 + 1) * sizeof(double) + (size_t)8 * R * sizeof(int); }
// ... of spectra_y: ny elements of pitch 2 TX, twice; ny twiddles; the sums
inline size_t lds_y(int ny, int TX, int G) { return ((size_t)4 * TX * ny + ny) * sizeof(cplx) + (size_t)G * NCH * (ny / 2 + 1) * sizeof(double) + (size_t)8 * TX * sizeof(int); }

inline int groups(int modes, int blk) { const int g = NT / modes; return g < 1 ? 1 : (g > blk ? blk : g); }

// rows per block (3D) or levels per workgroup (2D: `avail` = nz, no sums in LDS): the most, up to 32, within LDS_TARGET; 1 beyond it
inline Plan plan_x(int nx, int ny, int nz)
{
    Plan p{};
    const int avail = ny > 1 ? ny : nz;
    int R = avail < 32 ? avail : 32;
    auto need = [&](int r) { return lds_x(nx, r, ny > 1 ? groups(nx / 2 + 1, r) : 0); };
    while (R > 1 && need(R) > LDS_TARGET) --R;
    p.blk = R; p.G = ny > 1 ? groups(nx / 2 + 1, R) : 0; p.lds = need(R);
    return p;
}

inline Plan plan_y(int nx, int ny)
{
    Plan p{};
    int TX = nx < 32 ? nx : 32;
    auto need = [&](int c) { return lds_y(ny, c, groups(ny / 2 + 1, c)); };
    while (TX > 1 && need(TX) > LDS_TARGET) --TX;
    p.blk = TX; p.G = groups(ny / 2 + 1, TX); p.lds = need(TX);
    return p;
}

__device__ __forceinline__ RBC_SP_TARGET void barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// forward transform of `lines` lines of n = n1 * n2 values (line stride ls, element stride es) held in S; D: a second buffer of the
// same size.  Returns where the result is (D after the register-blocked transform, S after the generic one, whose scratch is
// lines * n dense values of D).  Both end with a barrier.  N1 > 0: n = 8 N1; N1 = 0: the generic routine.  A template argument of
// the kernels, chosen by the host: the transform sits in the kernels' loop over blocks, and with all variants in one kernel the
// constants of every one of them stay live across that loop (SGPR spills).
template <int N1>
__device__ __forceinline__ RBC_SP_TARGET const cplx *lines_fft(cplx *S, cplx *D, int lines, int n, int n1, int n2, int ls, int es, const cplx *tw)
{
    if constexpr (N1 > 0) {
        [[clang::always_inline]] rbc3::slab_fft<N1>(S, D, lines, ls, es, tw, -1);
        return D;
    } else {
        [[clang::always_inline]] rbc3::slab_dft(S, S, lines, n, n1, n2, ls, es, tw, -1, D);
        return S;
    }
}

// N1 of the register-blocked transform for this plan's length, 0 = generic: 4, 6, 8, and 12 along x.  Not every instantiation the
// pressure solve has: slab_fft and slab_dft are shared with its kernels, and the compiler specialises them over ALL their call sites
// before it inlines any.  A call of slab_fft<16> from here (either direction), or of slab_fft<12> with an element stride other than
// the 1 every other caller passes, changes the code of k2s_rhs_fft_pair / k2s_ifft_pair (68 -> 102 SGPRs, 216 -> 240 bytes of scratch:
// tests/test_kernel_resources.py) -- and spectra_x<., ., 16> itself was the one variant that spilled SGPRs.  Lines of 128 values,
// and of 96 along y, take the generic routine.
inline int fast_n1(const Plan &p, bool along_y)
{
    const bool fast = p.n2 == 8 && (p.n1 == 4 || p.n1 == 6 || p.n1 == 8 || (!along_y && p.n1 == 12));
    return fast ? p.n1 : 0;
}

// the two real lines f, g packed as z = f + i g, at mode m of n: 2 F = P + Q, 2 G = (P - Q) / i with P = z[m], Q = conj z[(n - m) mod n]
// mark[0], mark[1]: does f, does g hold a value other than 0?  A part that does not is 0 times its partner (header: a zero partner)
struct Pair { double fr, fi, gr, gi; };
__device__ __forceinline__ RBC_SP_TARGET Pair unpack(const cplx *z, int es, int n, int m, const int *mark)
{
    const cplx p = z[m * es], q = z[((m == 0) ? 0 : n - m) * es];
    Pair r{p.x + q.x, p.y - q.y, p.y + q.y, q.x - p.x};
    if (!mark[1]) r.gr = r.gi = 0.0 * (r.fr + r.fi);
    if (!mark[0]) r.fr = r.fi = 0.0 * (r.gr + r.gi);
    return r;
}

// staging: the value as float64, its line's mark set if it is not 0 (every writer stores the same 1: no atomic needed)
template <typename T>
__device__ __forceinline__ RBC_SP_TARGET double staged(T x, int *mark)
{
    const double d = (double)x;
    if (d != 0.0) *mark = 1;
    return d;
}

// the six (unscaled) terms of one row at one mode: bw = the line b + i w, uv = the line u + i v, mbw / muv their marks
__device__ __forceinline__ RBC_SP_TARGET void terms(const cplx *bw, const cplx *uv, int es, int n, int m, const int *mbw, const int *muv, double *s)
{
    const Pair a = unpack(bw, es, n, m, mbw), c = unpack(uv, es, n, m, muv);
    s[0] = a.fr * a.fr + a.fi * a.fi;
    s[1] = c.fr * c.fr + c.fi * c.fi;
    s[2] = c.gr * c.gr + c.gi * c.gi;
    s[3] = a.gr * a.gr + a.gi * a.gi;
    s[4] = a.fr * a.gr + a.fi * a.gi;        // Re (B conj W)
    s[5] = a.fi * a.gr - a.fr * a.gi;        // Im (B conj W)
}

// one-sided weight of mode m of n, times the 1/4 of the two halvings in `unpack`
__device__ __forceinline__ RBC_SP_TARGET double weight(int m, int n) { return (m == 0 || 2 * m == n) ? 0.25 : 0.5; }

// grid: B * nz workgroups (ny > 1) or B * ceil(nz / R) (2D handles), 256 threads; LDS lds_x.  px: [B][6][nz][nx/2 + 1]
template <typename T, bool HAS_V, int N1>
__global__ __launch_bounds__(NT) RBC_SP_TARGET void spectra_x(const Layout L, const Plan P, const T *__restrict__ state, const cplx *__restrict__ tw,
                                                              double *__restrict__ px)
{
    extern __shared__ __attribute__((aligned(16))) cplx sm[];
    const int nx = L.nx, ny = L.ny, nz = L.nz, nm = nx / 2 + 1, nxp = nx | 1, R = P.blk, G = P.G, t = threadIdx.x;
    const bool flat = ny == 1;                               // 2D handle: the workgroup's rows are R consecutive levels
    cplx *S = sm, *D = sm + 2 * R * nxp, *twx = sm + 4 * R * nxp;
    double *acc = reinterpret_cast<double *>(twx + nx);      // [g][ch][m], entry (g, ., m) owned by thread item g * nm + m
    int *marks = reinterpret_cast<int *>(acc + G * NCH * nm); // [block parity][line][part]: cleared for the next block while this one is read
    const int per_env = flat ? (nz + R - 1) / R : nz, env = blockIdx.x / per_env, kb = blockIdx.x - env * per_env;
    const int k0 = flat ? kb * R : kb, all_rows = flat ? ((nz - k0 < R) ? nz - k0 : R) : ny;
    const T *sb = state + (size_t)env * L.env_stride + (size_t)k0 * nx * ny;
    for (int i = t; i < nx; i += NT) twx[i] = tw[i];
    for (int i = t; i < G * NCH * nm; i += NT) acc[i] = 0.0;
    for (int i = t; i < 8 * R; i += NT) marks[i] = 0;
    barrier();
    const double rn = 1.0 / ((double)nx * (double)nx * (double)ny);
    double *out = px + ((size_t)env * NCH * nz + k0) * nm;    // channel stride nz * nm

    for (int j0 = 0; j0 < all_rows; j0 += R) {
        const int rows = (all_rows - j0 < R) ? all_rows - j0 : R;
        const T *b = sb + (size_t)j0 * nx, *u = b + L.ou, *w = b + L.ow;
        int *mk = marks + ((j0 / R) & 1) * 4 * R, *mk_next = marks + (((j0 / R) & 1) ^ 1) * 4 * R;
        for (int idx = t; idx < rows * nx; idx += NT) {
            const int l = idx / nx, i = idx - l * nx;
            double vv = 0.0;
            if constexpr (HAS_V) vv = staged(b[L.ov + idx], mk + 2 * (rows + l) + 1);
            S[l * nxp + i] = rbc3::make_real2(staged(b[idx], mk + 2 * l), staged(w[idx], mk + 2 * l + 1));
            S[(rows + l) * nxp + i] = rbc3::make_real2(staged(u[idx], mk + 2 * (rows + l)), vv);
        }
        barrier();
        for (int i = t; i < 4 * R; i += NT) mk_next[i] = 0;
        const cplx *Z = lines_fft<N1>(S, D, 2 * rows, nx, P.n1, P.n2, nxp, 1, twx);
        if (flat) {                                          // every row is a level of its own: nothing to add up
            for (int item = t; item < rows * nm; item += NT) {
                const int l = item / nm, m = item - l * nm;
                double s[NCH];
                terms(Z + l * nxp, Z + (rows + l) * nxp, 1, nx, m, mk + 2 * l, mk + 2 * (rows + l), s);
                const double sc = weight(m, nx) * rn;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) out[((size_t)ch * nz + l) * nm + m] = (!HAS_V && ch == 2) ? 0.0 : s[ch] * sc;
            }
        } else {
            for (int item = t; item < G * nm; item += NT) {
                const int g = item / nm, m = item - g * nm;
                double a[NCH], s[NCH];
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) a[ch] = acc[(g * NCH + ch) * nm + m];
                for (int l = g; l < rows; l += G) {         // ascending rows
                    terms(Z + l * nxp, Z + (rows + l) * nxp, 1, nx, m, mk + 2 * l, mk + 2 * (rows + l), s);
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) a[ch] += s[ch];
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) acc[(g * NCH + ch) * nm + m] = a[ch];
            }
        }
        barrier();                                           // the next block's staging overwrites the lines; the sums are complete
    }
    if (flat) return;
    for (int item = t; item < NCH * nm; item += NT) {
        const int ch = item / nm, m = item - ch * nm;
        double s = acc[ch * nm + m];
        for (int g = 1; g < G; ++g) s += acc[(g * NCH + ch) * nm + m];      // in group order
        out[(size_t)ch * nz * nm + m] = (!HAS_V && ch == 2) ? 0.0 : s * (weight(m, nx) * rn);
    }
}

// grid: B * nz workgroups, 256 threads; LDS lds_y.  py: [B][6][nz][ny/2 + 1]
template <typename T, int N1>
__global__ __launch_bounds__(NT) RBC_SP_TARGET void spectra_y(const Layout L, const Plan P, const T *__restrict__ state, const cplx *__restrict__ tw,
                                                              double *__restrict__ py)
{
    extern __shared__ __attribute__((aligned(16))) cplx sm[];
    const int nx = L.nx, ny = L.ny, nz = L.nz, nn = ny / 2 + 1, TX = P.blk, G = P.G, pitch = 2 * TX, t = threadIdx.x;
    cplx *S = sm, *D = sm + ny * pitch, *twy = sm + 2 * ny * pitch;
    double *acc = reinterpret_cast<double *>(twy + ny);      // [ch][n][g], entry (., n, g) owned by thread item n * G + g
    int *marks = reinterpret_cast<int *>(acc + G * NCH * nn); // [block parity][line][part], as in spectra_x
    const int env = blockIdx.x / nz, k = blockIdx.x - env * nz;
    const T *b = state + (size_t)env * L.env_stride + (size_t)k * nx * ny, *u = b + L.ou, *v = b + L.ov, *w = b + L.ow;
    for (int i = t; i < ny; i += NT) twy[i] = tw[nx + i];
    for (int i = t; i < G * NCH * nn; i += NT) acc[i] = 0.0;
    for (int i = t; i < 8 * TX; i += NT) marks[i] = 0;
    barrier();

    for (int x0 = 0; x0 < nx; x0 += TX) {
        const int cols = (nx - x0 < TX) ? nx - x0 : TX;
        int *mk = marks + ((x0 / TX) & 1) * 4 * TX, *mk_next = marks + (((x0 / TX) & 1) ^ 1) * 4 * TX;
        for (int idx = t; idx < ny * cols; idx += NT) {
            const int j = idx / cols, c = idx - j * cols, o = j * nx + x0 + c;
            S[j * pitch + c] = rbc3::make_real2(staged(b[o], mk + 2 * c), staged(w[o], mk + 2 * c + 1));
            S[j * pitch + cols + c] = rbc3::make_real2(staged(u[o], mk + 2 * (cols + c)), staged(v[o], mk + 2 * (cols + c) + 1));
        }
        barrier();
        for (int i = t; i < 4 * TX; i += NT) mk_next[i] = 0;
        const cplx *Z = lines_fft<N1>(S, D, 2 * cols, ny, P.n1, P.n2, 1, pitch, twy);
        for (int item = t; item < G * nn; item += NT) {
            const int n = item / G, g = item - n * G;        // lanes along columns
            double a[NCH], s[NCH];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) a[ch] = acc[(ch * nn + n) * G + g];
            for (int c = g; c < cols; c += G) {              // ascending columns
                terms(Z + c, Z + cols + c, pitch, ny, n, mk + 2 * c, mk + 2 * (cols + c), s);
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) a[ch] += s[ch];
            }
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) acc[(ch * nn + n) * G + g] = a[ch];
        }
        barrier();
    }
    const double rn = 1.0 / ((double)ny * (double)ny * (double)nx);
    double *out = py + ((size_t)env * NCH * nz + k) * nn;
    for (int item = t; item < NCH * nn; item += NT) {
        const int ch = item / nn, n = item - ch * nn;
        double s = acc[item * G];
        for (int g = 1; g < G; ++g) s += acc[item * G + g];                 // in group order
        out[(size_t)ch * nz * nn + n] = s * (weight(n, ny) * rn);
    }
}

// one launch on `stream`; `first`: the handle's first call, which lifts the kernel's dynamic-LDS limit to the CU's whole LDS (a
// ceiling, not a reservation: occupancy follows what a launch asks for)
template <typename K, typename... A>
inline hipError_t run(bool first, K kernel, unsigned grid, size_t lds, hipStream_t stream, A... args)
{
    if (first) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CEILING);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds, stream, args...);
    return hipGetLastError();
}


// the launches on `stream`; Y and py only for a 3D handle (HAS_V).  The plans' LDS sizes have been checked by the caller.
template <typename T, bool HAS_V>
inline hipError_t launch_spectra(bool first, const Layout &L, const Plan &X, const Plan &Y, const T *state, int B, const cplx *tw, double *px, double *py,
                                 hipStream_t stream)
{
    const unsigned per_env = (L.ny == 1) ? (unsigned)((L.nz + X.blk - 1) / X.blk) : (unsigned)L.nz;
    hipError_t e = hipSuccess;
#define RBC_SP_X(N1_) run(first, spectra_x<T, HAS_V, N1_>, (unsigned)B * per_env, X.lds, stream, L, X, state, tw, px)
    switch (fast_n1(X, false)) {
    case 4: e = RBC_SP_X(4); break;
    case 6: e = RBC_SP_X(6); break;
    case 8: e = RBC_SP_X(8); break;
    case 12: e = RBC_SP_X(12); break;
    default: e = RBC_SP_X(0); break;
    }
#undef RBC_SP_X
    if constexpr (HAS_V) {
        if (e != hipSuccess) return e;
#define RBC_SP_Y(N1_) run(first, spectra_y<T, N1_>, (unsigned)B * (unsigned)L.nz, Y.lds, stream, L, Y, state, tw, py)
        switch (fast_n1(Y, true)) {
        case 4: e = RBC_SP_Y(4); break;
        case 6: e = RBC_SP_Y(6); break;
        case 8: e = RBC_SP_Y(8); break;
        default: e = RBC_SP_Y(0); break;
        }
#undef RBC_SP_Y
    }
    return e;
}

}  // namespace rbcsp
