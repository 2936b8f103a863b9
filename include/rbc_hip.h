/*
 * rbc_hip.h -- C ABI of the MI355X-native batched Rayleigh-Benard stepper (librbc_hip.so).
 *
 * This is the drop-in boundary for the hot path of MichielStraat/RBC-Gym: it replaces the
 * Julia "plugin API" that the reference's gym envs call through juliacall
 *   src/rbc_gym/sim/rbc_sim2D_api.jl : initialize_simulation (:17), step_simulation (:75),
 *                                      get_state (:102), get_observation (:123),
 *                                      get_info (:134), get_nusselt (:142)
 * (call sites rbc2D.py:143,169,185,192,199,203-205) together with the un-vendored
 * Oceananigans.jl v0.92.0 solver underneath it (juliapkg.json:7-10).  Differences from the
 * reference interface, by design:
 *   - BATCHED: one handle owns B independent env instances resident in the HBM of one GPU
 *     (the reference holds one env in Julia module globals, one Julia runtime per env);
 *   - opaque handle instead of module globals; integer status + rbc_last_error() instead of
 *     Julia exceptions; nothing throws across the ABI;
 *   - arrays are C-order [env][channel][z][x] (what rbc2D.py produces AFTER its transposes),
 *     float32 for observations/state exactly like the Python boundary (rbc2D.py:185,192);
 *     all solver arithmetic is float64 like the reference.
 * Plain pointers and sizes only; no torch / HIP types in any signature (streams travel as
 * void*).  "_dev" entry points take DEVICE pointers (zero-copy PyTorch-ROCm tensors).
 *
 * Threading: calls on one handle must be serialised by the caller; different handles
 * (different GPUs) may be driven from different threads.  The library owns device state;
 * the caller owns every I/O buffer.
 */
#ifndef RBC_HIP_H
#define RBC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBC_ABI_VERSION 4

/* status codes */
enum {
    RBC_OK = 0,
    RBC_ERR_INVALID = 1,      /* bad argument / unsupported configuration              */
    RBC_ERR_DEVICE = 2,       /* HIP runtime error (message in rbc_last_error)         */
    RBC_ERR_NAN = 3,          /* at least one env produced NaNs (see rbc_get_flags)    */
    RBC_ERR_NOT_INITIALIZED = 4 /* step/get before the first reset (rbc_sim2D_api.jl:79-81) */
};

/* Mirrors the kwargs of initialize_simulation (rbc_sim2D_api.jl:17) plus the constants it
   hard-codes (:28-38).  Shapes are in the reference's Julia order (x, z). */
typedef struct rbc_config {
    int32_t abi_version;     /* = RBC_ABI_VERSION                                            */
    int32_t dim;             /* 2, or 3 (rbc_sim3D_api.jl: grid (nx,ny,nz), L (lx,ly,lz), heaters x heaters
                                actions, dt_* in free-fall units scaled by t_ff = lz^2, 4 channels b,u,v,w) */
    int32_t nx, ny, nz;      /* grid = state_shape[::-1]  (96, 1, 64).  dim=2, float64: any nx, nz >= 8 (the reference
                                takes any grid: rbc_sim2D_api.jl:17-25); the LDS-resident kernel where it is built for
                                the grid, the streaming kernels with ny = 1 otherwise.
                                dim=3: every direction >= 8.  Horizontal slabs that fit one workgroup's LDS (nx*ny <=
                                ~5000 in float64, ~10000 in float32) take the slab projection, larger ones the row /
                                pencil projection, whose bound is one (y, z) plane in LDS:
                                ny*nz <= ~5000 (float64), ~10000 (float32); beyond it rbc_create returns RBC_ERR_INVALID unless
                                `projection` below asks for the chunked y-z solve, whose bound is one line of y (128 x 128 x 64,
                                256 x 256 x 128, ... in either precision).  Every handle: batch * nx * ny * (nz + 1) < 2^31.
                                Tendencies: LDS tiles over full rows of x up to nx = 64, x- and y-tiled LDS tiles on wider grids
                                with nx % 32 == 0, ny % 8 == 0, nz % 4 == 0, the z-marching kernels otherwise
                                (rbc_debug_tendency_path tells which)                                                          */
    double  lx, ly, lz;      /* L = [2*pi, 2]                                   (api:28)     */
    double  ra;              /* default Rayleigh number for every env            (api:17)     */
    double  pr;              /* 0.7                                             (api:35)     */
    double  min_b, delta_b;  /* 1, 1                                            (api:30,36)  */
    int32_t heaters;         /* 12                                              (api:31)     */
    double  heater_limit;    /* 0.75                                            (api:32)     */
    double  dt_solver;       /* 0.03                                            (api:38)     */
    double  dt_control;      /* heater_duration = 1.5                           (api:33)     */
    double  random_kick;     /* 0.01                                            (api:37)     */
    int32_t obs_nx, obs_nz;  /* sensors = observation_shape[::-1] (48, 8)       (api:27)     */
    int32_t batch;           /* number of env instances B on this device                     */
    int32_t device;          /* HIP device ordinal                                           */
    int32_t write_state;     /* 1: rbc_step also refreshes the float32 full-state buffer     */
    int32_t precision;       /* arithmetic of the solver: RBC_PRECISION_F64 (0, the reference's Float64, default) or
                                RBC_PRECISION_F32 (1: float32 state and arithmetic) -- every path:
                                the LDS-resident 2D kernels, the streaming 2D grids and dim=3 (rbc3D.py:229-232 hands out
                                float32 observations anyway).  The I/O types of the ABI do not change with it (float64
                                fields in and out, float32 obs/state; Nusselt sums stay float64); only rbc_dev_fields()
                                exposes the solver's own element type (float for a float32 streaming / 3D handle).  */
    int32_t reference_clock; /* how many solver steps an env-step integrates (ABI 3).
                                RBC_CLOCK_DOCUMENTED (0, default): what the reference's SOURCES say -- run!(simulation) to
                                stop_time, stop_time += dt (rbc_sim2D_api.jl:84-85, rbc_sim3D_api.jl:88-89): every env-step
                                integrates dt_control, i.e. ceil(dt_control / dt_solver) solver steps.
                                RBC_CLOCK_RECORDED (1): what the reference's only RECORDED time series shows
                                (experiments/flowstats/flowstats_ra.pkl, written by flowstats_ra.py:55-66 through
                                rbc_sim3D_api.jl:77-101): the first env-step after a reset carries the growth of all its
                                solver steps, every later one of one solver step less (tau(n) = 1 + 0.98 (n - 1) at 50
                                solver steps per env-step on all four series).  With this value the
                                first rbc_step after a reset of an env integrates dt_control and every later one
                                dt_control - dt_solver (one full solver step dropped, a clipped last substep kept), while
                                t and step reported by rbc_get_info advance as documented.  Per env: a masked reset
                                restores the full first interval for the envs it resets, whatever the others are doing.
                                Needs dt_control > dt_solver.  dim = 2 and 3, every precision and path.                */
    int32_t projection;      /* dim = 3, which pressure projection the handle runs (ABI 4; ignored for dim = 2).
                                RBC_PROJECTION_AUTO (0, default): the slab kernels where a horizontal slab fits the LDS, the row /
                                pencil projection otherwise, refused beyond its (y, z) plane bound.
                                RBC_PROJECTION_PENCIL (1): the row / pencil projection on any 3D grid (what RBC_3D_PENCIL=1 forces).
                                RBC_PROJECTION_CHUNKED (2, or RBC_3D_PENCIL=2 in the environment): rows along x as in the pencil
                                projection, and the (y, z) plane walked in chunks of levels through memory instead of held in LDS
                                (DESIGN.md section 3b): bound ny <= ~2500 (float64), ~5100 (float32).  The chunk height follows from
                                the grid and the precision alone; RBC_PENCIL_CHUNK=<levels>, read by rbc_create, forces it.
                                Any other value: RBC_ERR_INVALID.                                                       */
} rbc_config;

enum { RBC_PRECISION_F64 = 0, RBC_PRECISION_F32 = 1 };
enum { RBC_CLOCK_DOCUMENTED = 0, RBC_CLOCK_RECORDED = 1 };
enum { RBC_PROJECTION_AUTO = 0, RBC_PROJECTION_PENCIL = 1, RBC_PROJECTION_CHUNKED = 2 };

typedef struct rbc_handle rbc_handle;

/* library / device */
int         rbc_abi_version(void);
const char *rbc_last_error(void);                 /* thread-local message of the last failure */
int         rbc_device_count(void);               /* number of visible HIP devices (0 if none) */
int         rbc_has_precision(int precision);     /* 1 if this build carries kernels for RBC_PRECISION_* */
void        rbc_default_config(rbc_config *cfg);  /* the gym registry defaults (__init__.py:7-18) */

/* lifetime: replaces gym.make()'s juliacall.newmodule + include (rbc2D.py:111-115) */
int  rbc_create(const rbc_config *cfg, rbc_handle **out);
int  rbc_destroy(rbc_handle *h);
/* Stream all launches of the handle go to.  NULL = the handle's own (non-blocking) stream, which has NO implicit ordering
   with any other stream: complete what the sim will read (actions written by another stream) before calling rbc_step_dev,
   and rbc_synchronize (or an event) before another stream reads the rbc_dev_* views.  To run ON the legacy default stream
   (what PyTorch's default stream, handle 0, is) pass hipStreamLegacy = (void*)1; any other value is a hipStream_t.      */
int  rbc_set_stream(rbc_handle *h, void *hip_stream);
void *rbc_get_stream(rbc_handle *h);
int  rbc_synchronize(rbc_handle *h);

/* per-env Rayleigh numbers (Ra sweep); ra[B] host pointer.  nu, kappa per api:40-41 */
int  rbc_set_rayleigh(rbc_handle *h, const double *ra);

/* RBCNormalizeObservation (wrappers/rbc_normalize_observation.py:66-74) fused into the observation write of
   the 2D step kernel: obs[c] = maxval * (2 * (obs[c] - min_vals[c]) / (max_vals[c] - min_vals[c]) - 1), evaluated
   in float32 in exactly that order on the float32-rounded sample, the python-float bounds rounded to float32 where
   numpy rounds them (bit-identical to the numpy wrapper), then
   clipped to [-maxval, maxval] if clip != 0 (a NaN stays a NaN, as with np.clip: a blown-up env is visible in its observation as
   well as in rbc_get_flags).  nch <= 5 channels (b,u,w,pHY',pNHS); channels >= nch stay raw;
   nch = 0 switches the transform off.  Takes effect from the next reset/step; rbc_get_state is never transformed.
   dim=3: nch <= 4 channels (b,u,v,w).  The 3D observation IS the float32 state buffer (rbc3D.py:229-232), so there the
   transform applies to what rbc_get_obs / rbc_get_state / rbc_dev_state hand out (rewritten at once for the current state);
   Nusselt number, NaN flag and rbc_get_fields3 always come from the raw float64 state. */
int  rbc_set_obs_normalization(rbc_handle *h, const double *min_vals, const double *max_vals, int nch, double maxval, int clip);

/* RBCRewardShaping.compute_cell_distances (wrappers/rbc_reward_shaping.py:85-140) on the device, for every env of a dim=2
   handle created with write_state=1: the largest periodic distance between two up-welling plumes (peaks of the float32
   vertical-velocity channel on the row nz/2 - 1 that reach `height`, the reference uses 0.001), 0 if the signal stays
   positive between them; domain length = cfg.lx.  out[B] float64 on the host; bit-identical to the numpy wrapper.
   rbc_dev_cell_dist: the device buffer the last call filled (NULL before the first call).
   rbc_debug_cell_distances: the same kernel on caller-provided host signals uy[B][nx] (parity tests).                  */
int   rbc_get_cell_distances(rbc_handle *h, double height, double *out);
void *rbc_dev_cell_dist(rbc_handle *h);
int   rbc_debug_cell_distances(int device, const float *uy, int B, int nx, double lx, double height, double *out);

/* render() of the 3D env (rbc3D.py:247-318) on the device: a volume ray-caster over the temperature field of the envs
   first_env .. first_env + n_envs - 1 of a dim=3 handle, read from the solver's own current state (float64 or float32; never the
   float32 observation buffer, so rbc_set_obs_normalization does not change the picture).  The picture is defined in DESIGN.md
   section 3c -- orthographic camera looking against view_from, point data on the box [0, (n-1) h] with the reference's y flip
   (rbc3D.py:275), samples every `step` plus one partial segment, trilinear interpolation, the caller's table lut[256][4] (float32
   RGBA in [0, 1], host pointer) read at 255 (T - clim[0]) / (clim[1] - clim[0]) with linear interpolation, segment opacity
   1 - (1 - a)^(length / unit), front-to-back compositing over bg -- and is NOT a pixel copy of VTK's output.
   step <= 0: half the smallest grid spacing; unit <= 0: box diagonal / (mean(nx, ny, nz) - 1).  A NaN sample is transparent.
   out: uint8 [n_envs][height][width][3] on the host, row 0 at the top.  Runs on the handle's stream behind the last step.
   RBC_ERR_INVALID: dim=2 handle; a null argument; width or height outside [1, 16384]; n_envs < 1, n_envs > 65535 or an env range
   outside the batch; view_from zero or not finite; clim not finite or clim[1] == clim[0]; bg not finite; a table entry outside
   [0, 1] (NaN included); step or unit not finite, or step shorter than box diagonal / 65536 (a ray never takes more samples than
   that); a grid with fewer than two points along an axis.  RBC_ERR_NOT_INITIALIZED before the first reset.
   rbc_dev_frames: the device buffer the last call filled (NULL before the first call).                                    */
typedef struct rbc_render3_params {
    int32_t width, height;
    double  view_from[3];    /* direction from the scene towards the camera                  */
    double  clim[2];
    double  step, unit;
    double  bg[3];
    int32_t first_env, n_envs;
} rbc_render3_params;
int   rbc_render3(rbc_handle *h, const rbc_render3_params *p, const float *lut, uint8_t *out);
void *rbc_dev_frames(rbc_handle *h);

/* Horizontal statistics of the current state, computed on the device from the solver's own float64 / float32 state (never from the
   float32 observation or state buffers: rbc_set_obs_normalization and write_state do not matter): what the reference's experiment
   records after every env-step (max |u|, |v|, |w| next to Nu, experiments/flowstats/flowstats_ra.py:64-67) and the row-wise
   moments of the profile pins (tests/profile_pins.py::row_moments_batch), extended to 3D.  Raw staggered values, no interpolation;
   level k = cell level k for b, u, v and face k (the bottom face of cell k, face 0 is the wall) for w.
   prof[e][m][k], float64 [B][6][nz]: the mean over the nx * ny cells of level k of  m = 0: b, 1: u^2, 2: v^2 (exactly 0 for dim = 2),
   3: w^2, 4: b w (cell k times its bottom face, the product of the Nusselt sum), 5: b^2.
   ext[e], float64 [B][5]: max |u|, max |v| (0 for dim = 2), max |w| (all nz + 1 faces), min b, max b over the env.
   Every product and sum is formed in float64 (a float32 handle's values are converted first), so the result is a pure function of
   what rbc_get_fields / rbc_get_fields3 return; an env's numbers do not depend on the batch.  A moment whose level holds a NaN in
   one of its fields is NaN, and so is an extremum of a field that holds a NaN anywhere in the env (numpy's mean / max / min).
   prof, ext: host pointers, either may be NULL (both NULL: the call returns without waiting, results stay on the device).  Runs on
   the handle's stream behind the last step; not recorded by rbc_set_profiling.  RBC_ERR_NOT_INITIALIZED before the first reset.
   rbc_dev_flowstats: the device buffers the last call filled, which = 0: prof, 1: ext (NULL before the first call; any other
   `which`: NULL, and rbc_last_error says so).                                                                              */
int   rbc_get_flowstats(rbc_handle *h, double *prof, double *ext);
void *rbc_dev_flowstats(rbc_handle *h, int which);

/* Horizontal power and co-spectra of the current state, level by level, computed on the device from the same buffer and under the
   same conventions as rbc_get_flowstats (raw staggered values; level k = cell level k of b, u, v and face k, the bottom face of cell
   k, of w; float64 throughout, a float32 state is widened first).  DESIGN.md section 3e.
   Line transform of row j of a level: F_j[m] = (1/nx) sum_i f[j][i] e^{-2 pi i m i / nx}, m = 0 .. nx/2 (numpy's rfft / nx); one-sided
   weights c_0 = 1, c_m = 2, c_{nx/2} = 1 for even nx.
   px[e][ch][k][m], float64 [B][6][nz][nx/2 + 1]:  ch 0: c_m mean_j |B_j[m]|^2;  1, 2, 3: the same for u, v (exactly 0 on a dim = 2
   handle: written, not computed), w;  4: co-spectrum c_m mean_j Re (B_j[m] conj W_j[m]);  5: quadrature spectrum, Im of the same.
   sum_m of ch 0, 1, 2, 3, 4 = prof[e][5, 1, 2, 3, 4][k] of rbc_get_flowstats (Parseval); for ny = 1, ch 4 and 5 over sqrt(ch 0 ch 3)
   are the cos and sin of the b-w cross phase.
   py[e][ch][k][n], float64 [B][6][nz][ny/2 + 1], dim = 3 only: the same six with the transform along y and the mean over x.
   NaN: b and w are transformed as one complex line, u and v as another, so a NaN in b or w of a level makes channels 0, 3, 4, 5 of
   that level NaN at every mode (in px and py), one in u or v channels 1 and 2 (dim = 2: 1 only); nothing else changes by a bit.
   (numpy would keep the partner's channel finite.)  An env's numbers do not depend on the batch.
   px, py: host pointers, either may be NULL (both NULL: the call returns without waiting, results stay on the device).  Runs on the
   handle's stream behind the last step; not recorded by rbc_set_profiling.  RBC_ERR_NOT_INITIALIZED before the first reset;
   RBC_ERR_INVALID for a non-NULL py on a dim = 2 handle, and where the two complex line sets of one row (one column) do not fit
   the 160 KB of LDS (nx, ny <= ~1500).
   rbc_dev_spectra: the device buffers the last call filled, which = 0: px, 1: py (NULL before the first call and for py of a
   dim = 2 handle; any other `which`: NULL, and rbc_last_error says so).                                                      */
int   rbc_get_spectra(rbc_handle *h, double *px, double *py);
void *rbc_dev_spectra(rbc_handle *h, int which);

/* Dissipation rates and velocity-gradient statistics of the current state, level by level, computed on the device from the same
   buffer and under the same conventions as rbc_get_flowstats (float64 throughout, a float32 state is widened first; the float32
   observation and state buffers are never read).  DESIGN.md section 3f.
   Grid: uniform, dx = lx/nx, dy = ly/ny, dz = lz/nz; u[i] the west face of cell i, v[j] the south face, w[k] the bottom face of
   cell k; x and y periodic.  Difference quotients at their natural staggered places:
     on level k = 0 .. nz-1:  dx b = (b[i] - b[i-1])/dx on x-faces, dy b on y-faces;  dx u = (u[i+1] - u[i])/dx, dy v and
                              dz w = (w[k+1] - w[k])/dz at centres;  dy u = (u[j] - u[j-1])/dy and dx v = (v[i] - v[i-1])/dx on xy-edges;
     on z-face k = 0 .. nz:   dz b = (b[k] - b[k-1])/dz;  dz u and dx w = (w[k][i] - w[k][i-1])/dx on xz-edges;  dz v and dy w on yz-edges;
     at the walls (no-slip, fixed temperature):  dz u = 2 u[0]/dz at face 0, -2 u[nz-1]/dz at face nz (likewise v);  w's wall faces
                              are what the state holds;  dz b = 2 (b[0] - wall_b)/dz at face 0, 2 (min_b - b[nz-1])/dz at face nz.
   wall_b: the bottom plate's temperature, float64 [B][ny][nx] on the host (ny = 1 for dim = 2); NULL = the uniform plate
   min_b + delta_b.  (The handle does not know the heater profile of the last step; the call does not guess it.)
   Outputs, means over the nx * ny points of a level; no viscosity or diffusivity enters:
     cells[e][c][k], float64 [B][4][nz]:    c = 0: (dx b)^2 + (dy b)^2;  1: (dx u)^2 + (dy v)^2 + (dz w)^2;  2: (dy u)^2 + (dx v)^2;
                                            3: dy u dx v
     faces[e][f][k], float64 [B][5][nz+1]:  f = 0: (dz b)^2;  1: (dz u)^2 + (dx w)^2;  2: dz u dx w;  3: (dz v)^2 + (dy w)^2;  4: dz v dy w
     tot[e][0..3], float64 [B][4]: volume means, every level with weight 1/nz, faces 0 and nz with half of it:
                                            0: |grad b|^2 = cells 0 + faces 0;  1: normal part, cells 1;  2: shear part, cells 2 +
                                            faces 1 + faces 3;  3: cross part, cells 3 + faces 2 + faces 4
   so that  eps_T = kappa tot0,  eps_u = nu (tot1 + tot2)  (strain form: nu (2 tot1 + tot2 + 2 tot3)),  enstrophy = tot2 - 2 tot3.
   On a dim = 2 handle every y-derivative and every v term is an exact zero, written and not computed (cells 2, 3 and faces 3, 4;
   cells 0, 1 lose their y parts); no v block is read.  A NaN makes NaN exactly the levels and faces whose stencil touches it, and tot
   through them; nothing else changes by a bit.  An env's numbers do not depend on the batch.
   cells, faces, tot: host pointers, any may be NULL (all NULL: the call returns without waiting, results stay on the device).  Runs
   on the handle's stream behind the last step; not recorded by rbc_set_profiling.  RBC_ERR_NOT_INITIALIZED before the first reset;
   RBC_ERR_INVALID where one row of a level does not fit a workgroup (nx > 2048), checked before anything is launched.
   rbc_dev_dissipation: the device buffers the last call filled, which = 0: cells, 1: faces, 2: tot (NULL before the first call; any
   other `which`: NULL, and rbc_last_error says so).                                                                          */
int   rbc_get_dissipation(rbc_handle *h, const double *wall_b, double *cells, double *faces, double *tot);
void *rbc_dev_dissipation(rbc_handle *h, int which);

/* Page-locked host buffers for the rbc_get_* outputs: a pinned destination takes the float32 state copy of 1024 envs (75 MB)
   at PCIe speed.  Plain helpers over hipHostMalloc / hipHostFree; any rbc_get_* accepts either kind of pointer.  Into PAGEABLE
   memory, rbc_get_obs / rbc_get_state outputs of 8 MiB and more are staged in chunks through a page-locked buffer of the handle
   and moved on by up to four host threads while the next chunk is in flight (RBC_STAGED_COPY=0: one hipMemcpy2D).      */
void *rbc_host_alloc(size_t bytes);
void  rbc_host_free(void *p);

/* initialize_simulation (api:17-70).  mask[B] (NULL = all): which envs to reset.
   Random IC (rbc_sim2D.jl:163-171) from the library's counter-based RNG, seeds[B].        */
int  rbc_reset(rbc_handle *h, const uint8_t *mask, const uint64_t *seeds);
/* checkpoint / identical-IC path (initialize_from_checkpoint, rbc_sim2D.jl:173-186):
   host arrays b,u: [B][nz][nx], w: [B][nz+1][nx] float64; only masked envs are read.      */
int  rbc_reset_from_arrays(rbc_handle *h, const uint8_t *mask,
                           const double *b, const double *u, const double *w);

/* 3D variants (initialize_from_checkpoint rbc_sim3D.jl:181-199; get_state rbc_sim3D_api.jl:106-121):
   b,u,v: [B][nz][ny][nx], w: [B][nz+1][ny][nx] float64                                      */
int  rbc_reset_from_arrays3(rbc_handle *h, const uint8_t *mask,
                            const double *b, const double *u, const double *v, const double *w);
int  rbc_get_fields3(rbc_handle *h, double *b, double *u, double *v, double *w);

/* step_simulation (api:75-97): actions [B][heaters] float32 in [-1,1] (host pointer;
   dim=3: [B][heaters][heaters], preprocess_action rbc_sim3D.jl:111-128 is applied on the device).
   Advances every env by dt_control. Returns RBC_OK, or RBC_ERR_NAN if any env has NaNs.   */
int  rbc_step(rbc_handle *h, const float *actions);
int  rbc_step_dev(rbc_handle *h, const float *actions_dev);  /* async on the handle's stream */

/* get_observation (api:123-129) after rbc2D.py:191-196: [B][nch][obs_nz][obs_nx] float32,
   channels b,u,w,(pHY',pNHS); nch = 3 or 5.                                               */
int  rbc_get_obs(rbc_handle *h, float *out, int nch);
/* get_state (api:102-118) after rbc2D.py:184-189: [B][nch][nz][nx] float32                */
int  rbc_get_state(rbc_handle *h, float *out, int nch);
/* raw float64 prognostic fields (checkpoint writer / parity tests): b,u [B][nz][nx], w [B][nz+1][nx] */
int  rbc_get_fields(rbc_handle *h, double *b, double *u, double *w);
/* get_nusselt (api:142-163): nu_state[B], nu_obs[B] float64 (either may be NULL)          */
int  rbc_get_nusselt(rbc_handle *h, double *nu_state, double *nu_obs);
/* get_info (api:134-137): t[B] float64, step[B] int64                                     */
int  rbc_get_info(rbc_handle *h, double *t, int64_t *step);
/* step_contains_NaNs (rbc_sim2D.jl:223-228): flags[B], 1 = NaN in b,u or w                */
int  rbc_get_flags(rbc_handle *h, int32_t *flags);

/* device-resident views for zero-copy consumers (valid until rbc_destroy):
   obs float32 [B][5][obs_nz][obs_nx], state float32 [B][5][nz][nx],
   nusselt float64 [B][2] (state, obs), flags int32 [B]                                    */
void *rbc_dev_obs(rbc_handle *h);
void *rbc_dev_state(rbc_handle *h);
void *rbc_dev_nusselt(rbc_handle *h);
void *rbc_dev_flags(rbc_handle *h);
void *rbc_dev_fields(rbc_handle *h);   /* float64 [B][ b(nz*nx) | u(nz*nx) | w((nz+1)*nx) ]; 2D handles on the streaming path
                                          (grids without an LDS-resident kernel): [B][ b | u | v = 0 | w ] of the buffer that
                                          currently holds the state (it alternates between two with every RK3 stage) */

/* measurement support for bench.py: HIP events are recorded on the handle's stream around
   every step-kernel launch of rbc_step / rbc_step_dev and the kernel of rbc_render3 (up to max_launches launches between
   two reads; 0 disables).  rbc_profile_read waits for the recorded launches, writes their
   durations in milliseconds to ms[0..capacity) and returns how many it wrote (-1 on error).  The durations come in issue
   order and carry no tag: a caller that steps AND renders between two reads gets both kinds mixed -- read (or switch
   profiling off) before rendering if only step times are wanted. */
int    rbc_set_profiling(rbc_handle *h, int max_launches);
int    rbc_profile_read(rbc_handle *h, double *ms, int capacity);
/* On-box streaming ceiling to report next to the 8 TB/s spec: copies `bytes` (rounded down to 16) from one
   device buffer to another `iters` times after a warm-up, with a 16-bytes-per-lane grid-stride copy kernel (best of five grid
   sizes) and with hipMemcpyAsync device-to-device; rates in GB/s count bytes read + bytes written.  Either output may be NULL.   */
int    rbc_copy_ceiling(int device, size_t bytes, int iters, double *kernel_gbs, double *memcpy_gbs);
/* algorithmic HBM bytes of one env-step per env under SURVEY.md 8(d)'s convention          */
double rbc_algorithmic_bytes_per_env_step(rbc_handle *h);

/* operator-level test hooks (used by the parity tests only; not needed by the env layer):
   tendencies G(b,u,w) of the current state for the given actions: gb,gu,gw [B][nz][nx]    */
int  rbc_debug_tendencies(rbc_handle *h, const float *actions, double *gb, double *gu, double *gw);
int  rbc_debug_tendencies3(rbc_handle *h, const float *actions, double *gu, double *gv, double *gw, double *gb);
/* run `nsub` RK3 substeps of size dt with the given actions (no counters touched)          */
int  rbc_debug_substeps(rbc_handle *h, const float *actions, int nsub, double dt);
/* how the streaming path (3D, streaming 2D) replays an env-step: groups[0] = env groups (stream chains) of the handle, groups[1] =
   1 if every group replays its own captured graph on a stream with a hardware queue of its own (found by probing at rbc_create), 0 if
   the groups are branches of one graph (or launches are direct).  A handle on the LDS-resident 2D kernel reports {1, 0}.          */
int  rbc_debug_launch_plan(rbc_handle *h, int groups[2]);
/* which tendency kernels the handle's stage plan launches (what the step selects, not a re-derivation): *path = 0 cell-per-thread,
   1 z-marching, 2 LDS tiles over full rows of x, 3 flat tiles (streaming 2D), 4 x- and y-tiled LDS tiles (grids wider than 64 cells);
   -1 for a handle on the LDS-resident 2D kernel.  Environment, read when a step is issued: RBC_NO_TILE=1 no tile kernel at all,
   RBC_TILE_SHAPE=16x16|16x8|16x4|8x8 forces a full-row shape, RBC_TILE_X=0 keeps wide grids on the z-marching kernels, RBC_TILE_X=1
   takes the x-tiled kernel on every 3D grid with nx % 32 == 0, ny % 8 == 0, nz % 4 == 0 (nx <= 64 included).                      */
int  rbc_debug_tendency_path(rbc_handle *h, int *path);
/* which pressure projection the handle's stage plan launches: *path = 0 slab kernels, 1 row / pencil projection with the one-plane
   y-z solve, 2 with the chunked y-z solve; -1 for a handle on the LDS-resident 2D kernel or on the streaming 2D path.        */
int  rbc_debug_projection_path(rbc_handle *h, int *path);
/* diagnostic builds only (-DRBC_STAMPS=1): per-phase shader-clock cycles of the last launch,
   out[B][64]; returns RBC_ERR_INVALID in the shipped build                                 */
int  rbc_debug_stamps(rbc_handle *h, unsigned long long *out);

#ifdef __cplusplus
}
#endif
#endif
