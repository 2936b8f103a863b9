// rbc_dissipation.hpp -- velocity- and temperature-gradient statistics of the solver's state on the device (gfx950); included by
// rbc_api.hip.  DESIGN.md section 3f and include/rbc_hip.h (rbc_get_dissipation) have the definitions; in short, for env e
//   cells[e][0..3][k], k = 0 .. nz - 1: level means of (dx b)^2 + (dy b)^2, (dx u)^2 + (dy v)^2 + (dz w)^2, (dy u)^2 + (dx v)^2, dy u dx v
//   faces[e][0..4][k], k = 0 .. nz:     level means of (dz b)^2, (dz u)^2 + (dx w)^2, dz u dx w, (dz v)^2 + (dy w)^2, dz v dy w
//   tot[e][0..3]: their volume means (faces 0 and nz with weight 1/2)
// every difference quotient at its natural place of the C grid, no-slip / fixed-temperature ghost values at the two walls, float64
// throughout (a float32 state is widened first; differences of widened values are the differences numpy forms).
//
// A Z-MARCHING STENCIL REDUCTION.  A workgroup owns one y-strip of one z-chunk of one env; a thread owns up to CPT columns (j, i)
// of the strip -- cell c = q NT + t of the strip, q = 0 .. CPT - 1, row-major -- and marches upward:
//   registers: the PREVIOUS level's b, u, v of its columns (every dz needs no LDS and no second read) and w one level AHEAD (dz w of
//              this level; it becomes the next level's w);
//   LDS:       the CURRENT level's b, u, v, w of the strip, once, for the periodic i - 1 / i + 1 / j - 1 / j + 1 neighbours, with one
//              halo row (row j0 - 1 of b, u, w; row j1 of v) re-read from memory.
// Every state value is loaded once, apart from the halo rows and the one level a chunk re-reads to prime its registers.
// The split reads the GRID alone, never the batch: levels of up to SMALL_LEVEL cells go to one wave per (env, chunk) (NW = 1: no
// workgroup barrier, the LDS lines are wave-private), larger planes to eight waves per (env, chunk, strip), the plane cut into
// the fewest strips of equal height whose cells fit the threads' registers (TILE = 8 * 64 * CPT); chunks are ZC levels, so that
// a batch of 32 envs of 48 x 48 x 32 is 512 workgroups instead of 32.  One row must fit the tile (nx <= 2048, 128 KB of LDS with
// its halo): checked on the host before anything is launched.
// The nine sums of a level are reduced by the fixed butterfly of rbc_flowstats.hpp and across the waves in wave order through
// LDS; strip partials go to part[e][strip][9][nz + 1], and dissipation_fold, a second small launch, adds them in strip order, divides
// by n_h and folds tot in level order.  No atomics, no arrival counters, nothing between workgroups.  Which thread adds which
// value is fixed by row, column and level numbers, every load is one element wide: an env's bits do not depend on the batch, on
// its position in it or on alignment.  NaNs go where the sums put them.
#pragma once
#include "rbc_flowstats.hpp"

namespace rbcds {

using rbcfs::WAVE;
using rbcfs::xor_lane;

constexpr int CPT = 4;                    // columns per thread (registers: 4 CPT values of the march, 4 CPT of the level, 9 float64 sums)
constexpr int ZC = 4;                     // levels per z-chunk
constexpr int NW_BIG = 8;                 // waves per workgroup of the strip variant
constexpr int SMALL_LEVEL = WAVE * CPT;   // cells per level up to which one wave owns the level
constexpr int TILE = NW_BIG * WAVE * CPT; // cells per strip
constexpr int NCELL = 4, NFACE = 5, NCH = NCELL + NFACE;
constexpr size_t LDS_CEILING = 160 * 1024;

struct Plan {
    size_t env_stride, ou, ov, ow;        // where u, v, w of one env sit in the state buffer, in elements (resident 2D: no v block)
    int nx, ny, nz, n_h;
    int nw, rows, nstrips, nchunks;       // waves per workgroup, rows per strip, strips per level, chunks per column
    unsigned lds;                         // bytes: the fields' lines, then red[nw][NCH]
    double rdx, rdy, rdz, min_b, wall_b;  // wall_b: the uniform plate min_b + delta_b (used where the caller passes no profile)
};

// every size known on the host before anything is allocated or launched; false: one row does not fit the tile
inline bool make_plan(Plan &P, int nx, int ny, int nz, size_t elem, bool has_v)
{
    P.nx = nx; P.ny = ny; P.nz = nz; P.n_h = nx * ny;
    P.nchunks = (nz + ZC - 1) / ZC;
    if (P.n_h <= SMALL_LEVEL) { P.nw = 1; P.nstrips = 1; P.rows = ny; }
    else {
        if (nx > TILE) return false;
        const int rmax = TILE / nx;
        P.nw = NW_BIG;
        P.nstrips = (ny + rmax - 1) / rmax;
        P.rows = (ny + P.nstrips - 1) / P.nstrips;
        P.nstrips = (ny + P.rows - 1) / P.rows;            // no empty strip
    }
    const size_t fields = (size_t)(has_v ? 4 : 3) * (P.rows + 1) * nx * elem;
    P.lds = (unsigned)((fields + 7) / 8 * 8 + (size_t)P.nw * NCH * sizeof(double));
    return P.lds <= LDS_CEILING;
}

// LDS writes of this workgroup are visible to its reads behind this point (NW = 1: the workgroup is one wave, no s_barrier)
template <int NW>
__device__ __forceinline__ RBC_FS_TARGET void sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if constexpr (NW > 1) __builtin_amdgcn_s_barrier();
    else __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// B * nchunks * nstrips workgroups of NW * 64 threads; part: [B][nstrips][9][nz + 1]; wall: [B][ny][nx] or nullptr
template <typename T, bool HAS_V, int NW>
__global__ __launch_bounds__(NW * WAVE) RBC_FS_TARGET void dissipation_march(const Plan P, const T *__restrict__ state, const double *__restrict__ wall,
                                                                            double *__restrict__ part)
{
    constexpr int NT = NW * WAVE;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int strip = blockIdx.x % P.nstrips, rest = blockIdx.x / P.nstrips, chunk = rest % P.nchunks, env = rest / P.nchunks;
    const int nx = P.nx, ny = P.ny, nz = P.nz, n_h = P.n_h;
    const bool yon = HAS_V && ny > 1;                         // a dim = 2 handle: no y-derivative, no v term, no v read
    const int j0 = strip * P.rows, nr = (P.rows < ny - j0) ? P.rows : ny - j0, ncs = nr * nx, g0 = j0 * nx;
    const int jm = (j0 == 0 ? ny : j0) - 1, jp = (j0 + nr == ny) ? 0 : j0 + nr;       // the halo rows: below b, u, w; above v
    // LDS lines of (rows + 1) * nx values: b, u, w hold the halo row first (own cell c at nx + c, its j - 1 neighbour at c), v the
    // own rows first (own cell c at c, its j + 1 neighbour at c + nx)
    const int fld = (P.rows + 1) * nx;
    T *sb = reinterpret_cast<T *>(lds_raw), *su = sb + fld, *sw = su + fld, *sv = sw + fld;
    double *red = reinterpret_cast<double *>(lds_raw + ((size_t)(HAS_V ? 4 : 3) * fld * sizeof(T) + 7) / 8 * 8);

    const T *gb = state + (size_t)env * P.env_stride, *gu = gb + P.ou, *gv = gb + P.ov, *gw = gb + P.ow;
    const int k0 = chunk * ZC, k1 = (k0 + ZC < nz) ? k0 + ZC : nz, kend = (k1 == nz) ? nz + 1 : k1;   // faces k0 .. kend - 1, levels k0 .. k1 - 1
    const double rdx = P.rdx, rdy = P.rdy, rdz = P.rdz;

    int col[CPT];
    T pb[CPT], pu[CPT], pv[CPT], wn[CPT];                     // the level below (b, u, v) and the face ahead (w)
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
        const int c = q * NT + t;
        col[q] = c % nx;
        pb[q] = pu[q] = pv[q] = wn[q] = (T)0;
        if (c < ncs) {
            wn[q] = gw[(size_t)k0 * n_h + g0 + c];
            if (k0 > 0) {
                const size_t o = (size_t)(k0 - 1) * n_h + g0 + c;
                pb[q] = gb[o]; pu[q] = gu[o];
                if (yon) pv[q] = gv[o];
            }
        }
    }

    for (int k = k0; k < kend; ++k) {
        const bool lev = k < nz;                               // face nz has no cell level above it
        const size_t ok = (size_t)k * n_h;
        T cb[CPT], cu[CPT], cv[CPT], cw[CPT];
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            const int c = q * NT + t;
            cb[q] = cu[q] = cv[q] = (T)0;
            cw[q] = wn[q];
            if (c < ncs) {
                sw[nx + c] = cw[q];
                if (lev) {
                    cb[q] = gb[ok + g0 + c]; cu[q] = gu[ok + g0 + c];
                    wn[q] = gw[ok + n_h + g0 + c];
                    sb[nx + c] = cb[q]; su[nx + c] = cu[q];
                    if (yon) { cv[q] = gv[ok + g0 + c]; sv[c] = cv[q]; }
                }
            }
        }
        if (yon)
            for (int i = t; i < nx; i += NT) {
                sw[i] = gw[ok + (size_t)jm * nx + i];
                if (lev) {
                    sb[i] = gb[ok + (size_t)jm * nx + i]; su[i] = gu[ok + (size_t)jm * nx + i];
                    sv[ncs + i] = gv[ok + (size_t)jp * nx + i];
                }
            }
        sync<NW>();

        double a[NCH];
#pragma unroll
        for (int m = 0; m < NCH; ++m) a[m] = 0.0;
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            const int c = q * NT + t;
            if (c >= ncs) continue;
            const int im = c + (col[q] == 0 ? nx - 1 : -1), ip = c + (col[q] == nx - 1 ? 1 - nx : 1);
            const double b = (double)cb[q], u = (double)cu[q], v = (double)cv[q], w = (double)cw[q];
            // face k: the wall faces take the ghost values of the Value boundary conditions
            double dzb, dzu, dzv;
            if (k == 0) {
                const double wb = wall ? wall[(size_t)env * n_h + g0 + c] : P.wall_b;
                dzb = (2.0 * (b - wb)) * rdz; dzu = (2.0 * u) * rdz; dzv = (2.0 * v) * rdz;
            } else if (k == nz) {
                dzb = (2.0 * (P.min_b - (double)pb[q])) * rdz; dzu = (-2.0 * (double)pu[q]) * rdz; dzv = (-2.0 * (double)pv[q]) * rdz;
            } else {
                dzb = (b - (double)pb[q]) * rdz; dzu = (u - (double)pu[q]) * rdz; dzv = (v - (double)pv[q]) * rdz;
            }
            const double dxw = (w - (double)sw[nx + im]) * rdx;
            a[4] += dzb * dzb;
            a[5] += dzu * dzu + dxw * dxw;
            a[6] += dzu * dxw;
            if (yon) {
                const double dyw = (w - (double)sw[c]) * rdy;
                a[7] += dzv * dzv + dyw * dyw;
                a[8] += dzv * dyw;
            }
            if (lev) {
                const double dxb = (b - (double)sb[nx + im]) * rdx, dxu = ((double)su[nx + ip] - u) * rdx, dzw = ((double)wn[q] - w) * rdz;
                if (yon) {
                    const double dyb = (b - (double)sb[c]) * rdy, dyv = ((double)sv[c + nx] - v) * rdy;
                    const double dyu = (u - (double)su[c]) * rdy, dxv = (v - (double)sv[im]) * rdx;
                    a[0] += dxb * dxb + dyb * dyb;
                    a[1] += dxu * dxu + dyv * dyv + dzw * dzw;
                    a[2] += dyu * dyu + dxv * dxv;
                    a[3] += dyu * dxv;
                } else {
                    a[0] += dxb * dxb;
                    a[1] += dxu * dxu + dzw * dzw;
                }
                pb[q] = cb[q]; pu[q] = cu[q]; pv[q] = cv[q];
            }
        }

        // the wave's sums by the fixed butterfly (every lane takes part, whether it owns a column or not), then the waves in wave order
#pragma unroll
        for (int m = 0; m < NCH; ++m) {
            if (!yon && (m == 2 || m == 3 || m == 7 || m == 8)) continue;      // exact zeros stay what they are
            double s = a[m];
            s += xor_lane<1>(s, lane); s += xor_lane<2>(s, lane); s += xor_lane<4>(s, lane);
            s += xor_lane<8>(s, lane); s += xor_lane<16>(s, lane); s += xor_lane<32>(s, lane);
            a[m] = s;
        }
        double mine = 0.0;                                     // lane m carries channel m
#pragma unroll
        for (int m = 0; m < NCH; ++m)
            if (lane == m) mine = a[m];
        if constexpr (NW > 1) {
            if (lane < NCH) red[wave * NCH + lane] = mine;
            sync<NW>();                                        // also: every wave is done with the fields' lines of this level
            if (wave == 0 && lane < NCH) {
                mine = red[lane];
#pragma unroll
                for (int q = 1; q < NW; ++q) mine += red[q * NCH + lane];
            }
        }
        if (wave == 0 && lane < NCH && (lane >= NCELL || lev))
            part[(((size_t)env * P.nstrips + strip) * NCH + lane) * (nz + 1) + k] = mine;
    }
}

// one wave per env: cells[e][c][k] and faces[e][f][k] = the strips' partials added in strip order, over n_h; then tot[e][0..3], folded
// in level order by lanes 0 .. 3 from the values just written (faces 0 and nz with weight 1/2), over nz
__global__ __launch_bounds__(WAVE) RBC_FS_TARGET void dissipation_fold(const double *__restrict__ part, double *cells, double *faces, double *__restrict__ tot,
                                                                       int nz, int nstrips, double n_h)
{
    const int env = blockIdx.x, lane = threadIdx.x, nf = nz + 1;
    double *ce = cells + (size_t)env * NCELL * nz, *fe = faces + (size_t)env * NFACE * nf;
    for (int idx = lane; idx < NCH * nf; idx += WAVE) {
        const int m = idx / nf, k = idx - m * nf;
        if (m < NCELL && k == nz) continue;
        const double *p = part + ((size_t)env * nstrips * NCH + m) * nf + k;
        double s = p[0];
        for (int st = 1; st < nstrips; ++st) s += p[(size_t)st * NCH * nf];
        s /= n_h;
        if (m < NCELL) ce[(size_t)m * nz + k] = s;
        else fe[(size_t)(m - NCELL) * nf + k] = s;
    }
    sync<1>();
    if (lane >= 4) return;
    // lane 0: |grad b|^2 = cells 0 + faces 0; 1: normal part, cells 1; 2: shear part, cells 2 + faces 1 + faces 3; 3: cross part,
    // cells 3 + faces 2 + faces 4
    const int fa = (lane == 0) ? 0 : (lane == 2) ? 1 : 2, fb = (lane == 2) ? 3 : 4;
    double acc = 0.0;
    for (int k = 0; k <= nz; ++k) {
        const double wk = (k == 0 || k == nz) ? 0.5 : 1.0;
        if (lane != 1) acc += wk * fe[(size_t)fa * nf + k];
        if (lane >= 2) acc += wk * fe[(size_t)fb * nf + k];
        if (k < nz) acc += ce[(size_t)lane * nz + k];
    }
    tot[(size_t)env * 4 + lane] = acc / (double)nz;
}

// both launches on `stream`.  HAS_V = false: the resident 2D layout [b | u | w]
template <typename T, bool HAS_V>
inline hipError_t launch_dissipation(const Plan &P, const T *state, const double *wall, int B, double *part, double *cells, double *faces, double *tot,
                                     hipStream_t stream)
{
    const dim3 grid((unsigned)B * (unsigned)P.nchunks * (unsigned)P.nstrips);
    if (P.lds > 64 * 1024) {       // per-kernel process state, a ceiling and not a reservation: the CU's whole LDS once (rbc3d_host_body.hpp)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dissipation_march<T, HAS_V, NW_BIG>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CEILING);
        if (e != hipSuccess) return e;
    }
    if (P.nw == 1) hipLaunchKernelGGL((dissipation_march<T, HAS_V, 1>), grid, dim3(WAVE), P.lds, stream, P, state, wall, part);
    else hipLaunchKernelGGL((dissipation_march<T, HAS_V, NW_BIG>), grid, dim3(NW_BIG * WAVE), P.lds, stream, P, state, wall, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dissipation_fold, dim3((unsigned)B), dim3(WAVE), 0, stream, part, cells, faces, tot, P.nz, P.nstrips, (double)P.n_h);
    return hipGetLastError();
}

}  // namespace rbcds
