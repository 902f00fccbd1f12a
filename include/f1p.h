/*
 * f1p.h -- C-ABI of libf1p.so, the MI355X (gfx950) batched trajectory-sampling planner.
 *
 * This is the drop-in boundary for the ONE data-parallel hot path of f1tenth/f1tenth_planning
 * (SURVEY.md section 8): pure-pursuit tracking, the lattice planner's sample -> clothoid -> cost ->
 * argmin -> track loop, and the kinematic-bicycle rollout of the kinematic MPC run as random shooting.
 * Every entry point names the reference interface (file:line under the reference tree) it replaces.
 * The reference is pure Python, so the binding a maintainer adds is a ctypes stub.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; `hipStream_t` never crosses the boundary;
 *   - every function returns 0 (F1P_OK) or a negative F1P_E* code and never throws or aborts;
 *     the message is available from f1p_last_error();
 *   - one ctx <-> one device <-> one HIP stream.  A ctx is not thread-safe; distinct ctxs are;
 *   - `*_batch`  : caller-owned HOST pointers, synchronous (H2D, kernels, D2H, stream sync);
 *     `*_dev`    : caller-owned DEVICE pointers (from f1p_dev_alloc), asynchronous on the ctx stream;
 *   - all floating-point payloads are IEEE binary64 unless the name says f32 -- the reference computes
 *     in numpy fp64 and the index decisions (nearest segment, look-ahead segment, best candidate) are
 *     required bit-exact;
 *   - row-major arrays, E = number of egos (independent vehicles) in the batch.
 */
#ifndef F1P_H
#define F1P_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F1P_VERSION_STRING "0.1.0"

/* error codes */
#define F1P_OK 0
#define F1P_EINVAL (-1)    /* bad argument (shape, NULL, range) -> ValueError in the shims            */
#define F1P_ENODEV (-2)    /* no usable HIP device / device index out of range                         */
#define F1P_EHIP (-3)      /* a HIP runtime call failed (message carries hipGetErrorString)            */
#define F1P_ESTATE (-4)    /* call order: waypoints / grid / communicator not set                      */
#define F1P_ENOMEM (-5)    /* device or host allocation failed                                         */
#define F1P_ECOMM (-6)     /* RCCL could not be loaded or a collective failed                          */

/* per-ego status written by the batch calls (a batch never fails because of one bad ego) */
#define F1P_ST_INTERSECT 0      /* look-ahead circle intersected the path   (pure_pursuit.py:70-79)   */
#define F1P_ST_REACQUIRE 1      /* nearest waypoint used, dist < max_reacquire (pure_pursuit.py:80-81) */
#define F1P_ST_NO_LOOKAHEAD 2   /* no look-ahead point: (0.0, 0.0) + warning (pure_pursuit.py:112-114) */
#define F1P_ST_ALL_BLOCKED 3    /* lattice: every candidate is in collision / infeasible               */
#define F1P_ST_BAD_TRACK 4      /* track-set calls: the ego's track id is outside [0, K) (NaN outputs)  */

/* candidate trajectory generators of the lattice planner */
#define F1P_GEN_CLOTHOID 0      /* G1 Hermite clothoid, what the reference builds with pyclothoids (lattice_planner.py:196) */
#define F1P_GEN_CUBIC 1         /* parametric cubic Hermite spline between the two poses (north_star "cubic-spline"):       */
                                /*   tangent magnitude = chord length, stations at equal parameter steps u_i = i/(S-1)       */

/* limits of the fixed-size config structs */
#define F1P_MAX_LOOKAHEADS 64
#define F1P_MAX_WIDTHS 64

typedef struct f1p_ctx f1p_ctx;

/* ------------------------------------------------------------------------------------------------
 * Lattice planner configuration.  Mirrors what the reference spreads over
 * LatticePlanner.plan (planning/lattice_planner/lattice_planner.py:174-214: 100 stations, tracker
 * look-ahead 0.8), sample_lookahead_square (:223-260: lookahead_distances, widths) and the example cost
 * functions (:268-296: inverse length, max |kappa|, mean |kappa|, heading similarity to the previous path).
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_lattice_cfg {
    int32_t n_stations;      /* S: stations per candidate, sample_traj npts (utils/utils.py:286-295); >= 2  */
    int32_t n_lookahead;     /* n_l: number of look-ahead distances (device-sampled goals)                  */
    int32_t n_width;         /* n_w: number of lateral offsets; candidates C = n_l * n_w, c = l*n_w + k     */
    int32_t n_shift;         /* N_SHIFT of get_similarity_cost (lattice_planner.py:287-296)                 */
    int32_t n_cull;          /* N_CULL  of get_similarity_cost; >= 0 here (0 keeps the whole tail)          */
    int32_t check_collision; /* 1: a station in an occupied / out-of-map cell makes the cost +inf           */
    int32_t cand_begin;      /* candidate shard [cand_begin, cand_begin + cand_count) evaluated by this     */
    int32_t cand_count;      /*   call; 0 count = all C (used when one ego's candidates span ranks)         */
    int32_t generator;       /* F1P_GEN_CLOTHOID (the reference's G1 clothoid, :196) or F1P_GEN_CUBIC             */
    int32_t prune;           /* 1: branch and bound over the candidates (clothoid generator, winner-only outputs):
                              * candidates whose cost lower bound exceeds the best cost found so far skip the
                              * station loop; every output is bit-identical to prune = 0                         */
    double lookahead[F1P_MAX_LOOKAHEADS]; /* metres, circle radii for intersect_point                       */
    double width[F1P_MAX_WIDTHS];         /* metres, lateral offsets along the path normal                  */
    double w_length;         /* weight of 1/L                 (get_length_cost     :268-271)                */
    double w_max_kappa;      /* weight of max_i |kappa(s_i)|  (get_max_curvature   :273-278)                */
    double w_mean_kappa;     /* weight of mean_i |kappa(s_i)| (get_mean_curvature  :280-285)                */
    double w_similarity;     /* weight of sum (theta_new - theta_prev)^2 (get_similarity_cost :287-296)     */
    double track_lookahead;  /* tracker look-ahead, 0.8 in the reference (lattice_planner.py:211)           */
    double wheelbase;        /* tracker wheelbase; the reference tracker uses 0.33 (lattice_planner.py:55)  */
    double max_reacquire;    /* PurePursuitPlanner.max_reacquire = 20.0 (pure_pursuit.py:52)                */
} f1p_lattice_cfg;

/* ------------------------------------------------------------------------------------------------
 * Kinematic-MPC shooting configuration: the numeric content of `mpc_config`
 * (control/kinematic_mpc/kinematic_mpc.py:40-68) that the rollout and the objective use.
 * State order is the reference's z = [x, y, v, yaw]; input order u = [accel, steer].
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_kmpc_cfg {
    int32_t horizon;         /* TK (8 in the reference, 30 in BASELINE config 4)                            */
    int32_t n_rollouts;      /* R candidate control sequences per ego                                       */
    double dt;               /* DTK = 0.1                                                                   */
    double wheelbase;        /* WB = 0.33                                                                   */
    double max_steer;        /* MAX_STEER = 0.4189 (MIN_STEER = -MAX_STEER)                                 */
    double max_dsteer;       /* MAX_DSTEER = pi rad/s; per-step bound is max_dsteer*dt (:391-394)           */
    double max_speed;        /* MAX_SPEED = 6                                                               */
    double min_speed;        /* MIN_SPEED = 0                                                               */
    double max_accel;        /* MAX_ACCEL = 3                                                               */
    double q[4];             /* diag Qk  = [13.5, 13.5, 5.5, 13.0]                                          */
    double qf[4];            /* diag Qfk = [13.5, 13.5, 5.5, 13.0]                                          */
    double r[2];             /* diag Rk  = [0.01, 100]                                                      */
    double rd[2];            /* diag Rdk = [0.01, 100]                                                      */
} f1p_kmpc_cfg;

/* ------------------------------------------------------------------------------------------------
 * Dynamic single-track shooting configuration: the numeric content of `mpc_config` of
 * control/dynamic_mpc/dynamic_mpc.py:40-86 that update_state (:317-404) and the objective (:616-622) use.
 * State z = [x, y, delta, v, yaw, yaw rate, beta]; input u = [steering speed, accel].
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_stmpc_cfg {
    int32_t horizon;         /* T = 40                                                                      */
    int32_t n_rollouts;      /* R candidate control sequences per ego                                       */
    double dt;               /* DT = 0.025                                                                  */
    double wheelbase;        /* WB = 0.33                                                                   */
    double max_steer;        /* MAX_STEER = 0.4189                                                          */
    double max_steer_v;      /* MAX_STEER_V = 3.2 rad/s (input bound AND the bound on its change, :685)     */
    double max_speed;        /* MAX_SPEED = 6                                                               */
    double min_speed;        /* MIN_SPEED = 0                                                               */
    double max_accel;        /* MAX_ACCEL = 3                                                               */
    double q[7];             /* diag Q  = [32, 32, 0, 1, 0.5, 0, 0]                                         */
    double qf[7];            /* diag Qf = [32, 32, 0, 1, 0.5, 0, 0]                                         */
    double r[2];             /* diag R  = [0.5, 0.01]  (steering speed, accel)                              */
    double rd[2];            /* diag Rd = [0.3, 0.01]                                                       */
    double params[8];        /* mass, l_f, l_r, h_CoG, c_f, c_r, Iz, mu  (STMPCPlanner.__init__ default)    */
} f1p_stmpc_cfg;
void f1p_stmpc_cfg_default(f1p_stmpc_cfg* cfg);

/* fill the structs with the reference defaults (lattice: 4 look-aheads x 7 widths, S = 100) */
void f1p_lattice_cfg_default(f1p_lattice_cfg* cfg);
void f1p_kmpc_cfg_default(f1p_kmpc_cfg* cfg);

/* ------------------------------------------------------------------------------------------------
 * Context, errors, device memory
 * ---------------------------------------------------------------------------------------------- */
const char* f1p_version(void);
/* number of visible HIP devices, or a negative error code.  Does not create a context. */
int f1p_device_count(void);
/* create a context bound to HIP device `device` (0-based) with its own non-blocking stream */
int f1p_create(f1p_ctx** out, int device);
void f1p_destroy(f1p_ctx* ctx);
/* last error message of this ctx (or of the last failed f1p_create when ctx == NULL) */
const char* f1p_last_error(const f1p_ctx* ctx);
/* device name / compute units / gcn arch string of the ctx device, for reports */
int f1p_device_info(const f1p_ctx* ctx, char* name, size_t name_len, int32_t* compute_units, char* arch, size_t arch_len);

/* caller-visible device buffers for the *_dev entry points (HBM-resident inputs / outputs) */
int f1p_dev_alloc(f1p_ctx* ctx, void** dptr, size_t bytes);
int f1p_dev_free(f1p_ctx* ctx, void* dptr);
int f1p_h2d(f1p_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);  /* async on the ctx stream */
int f1p_d2h(f1p_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);  /* async on the ctx stream */
int f1p_memset(f1p_ctx* ctx, void* dst_dev, int value, size_t bytes);          /* async on the ctx stream */
int f1p_sync(f1p_ctx* ctx);                                                    /* hipStreamSynchronize   */
/* page-locked host memory: the *_batch entry points DMA straight from / into such buffers instead of going through
 * the runtime's bounce buffers (a plan() that hands over pinned pose / result arrays saves ~0.1 ms per 4096 egos).
 * f1p_lattice_plan_batch goes further (round 6): with page-locked poses and result arrays -- 32 <= E < 8192 egos, device-sampled
 * goals, prev_theta NULL, the default schedule -- no copy is submitted at all: the first kernel reads the poses out of host memory
 * and the last one stores every result column and the best_traj rows where the caller reads them (p50 plan() at 4096 egos
 * 0.236 -> 0.218 ms, at 256 egos 0.090 -> 0.068).  The arrays must stay valid and unread until the call returns. */
int f1p_host_alloc(f1p_ctx* ctx, void** hptr, size_t bytes);
int f1p_host_free(f1p_ctx* ctx, void* hptr);

/* HIP-event timing on the ctx stream (the stream the kernels are launched on):
 * f1p_timer_begin records an event, f1p_timer_end records a second one, synchronises it and returns the
 * elapsed milliseconds between the two. */
int f1p_timer_begin(f1p_ctx* ctx);
int f1p_timer_end(f1p_ctx* ctx, float* elapsed_ms);

/* ------------------------------------------------------------------------------------------------
 * Static scene: waypoints (raceline / centreline) and the occupancy grid.  Copied to the device; no host
 * pointer is retained.  Replaces the `self.waypoints` attribute of every planner
 * (pure_pursuit.py:51-54, lattice_planner.py:44-49) and the `map` argument of the stub
 * map_collision (utils/utils.py:297-301).
 * ---------------------------------------------------------------------------------------------- */
/* wp: row-major [n][ncols] fp64; col_* select x, y, speed, heading.  col_psi < 0: no heading column
 * (pure pursuit only).  Pure pursuit / lattice rows are [x, y, v, psi, kappa]
 * (examples/control/Spielberg_raceline.csv:1), i.e. cols 0,1,2,3. */
int f1p_set_waypoints(f1p_ctx* ctx, const double* wp, int32_t n, int32_t ncols, int32_t col_x, int32_t col_y,
                      int32_t col_v, int32_t col_psi);
/* Same, with a curvature column (LQR feed-forward, control/lqr/lqr.py:93): rows [x, y, v, psi, kappa]
 * (examples/control/Spielberg_raceline.csv:1).  col_kappa < 0: none. */
int f1p_set_waypoints_ex(f1p_ctx* ctx, const double* wp, int32_t n, int32_t ncols, int32_t col_x, int32_t col_y,
                         int32_t col_v, int32_t col_psi, int32_t col_kappa);
/* img: row-major [h][w] u8, row 0 = TOP of the image (ROS map_server layout,
 * examples/control/Spielberg_map.yaml:1-6); cell (gx, gy) with gx = floor((x-ox)/res), gy = floor((y-oy)/res)
 * reads img[h-1-gy][gx]; a cell is occupied iff its value < occupied_below; outside the image is occupied. */
int f1p_set_grid(f1p_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, double res, double ox, double oy,
                 int32_t occupied_below);

/* Occupancy -> distance-transform preprocessor (the reference's collision hook is the stub
 * map_collision(points, map), utils/utils.py:297-301, and its vehicle is 0.58 m x 0.31 m, kinematic_mpc.py:60-61).
 * dist: row-major [h][w] f32 in the image's row order (row 0 = top): Euclidean distance in metres between cell centres
 * from every cell to the nearest occupied cell of the grid installed by f1p_set_grid (0 on occupied cells; cells
 * outside the image count as occupied, like the collision test), saturated at cap_cells * resolution.  The squared
 * distance in cells is an exact integer, so the result is bit-identical to the CPU restatement. */
int f1p_grid_distance_batch(f1p_ctx* ctx, float* dist, int32_t cap_cells);
/* Make the collision test footprint-aware: the active bitmap becomes the uploaded grid dilated by a disc of `radius`
 * metres (a cell is occupied iff its distance to an occupied cell is < radius), so the point test of every station is a
 * disc test.  radius = 0 restores the uploaded grid.  Planning kernels are unchanged.  With a footprint installed
 * (f1p_set_footprint) the dilation is radius + the footprint's disc radius: the two add, neither replaces the other. */
int f1p_inflate_grid(f1p_ctx* ctx, double radius);

/* Oriented vehicle footprint (the reference's vehicle is LENGTH 0.58 m x WIDTH 0.31 m, kinematic_mpc.py:60-61; its collision hook
 * map_collision, utils/utils.py:297-301, is a stub): the footprint is covered by n_discs discs of `radius` whose centres sit at
 * longitudinal `offsets` [m] from the pose along its heading.  The bitmap is dilated by `radius` ON TOP OF the inflation the caller
 * configured with f1p_inflate_grid (one exact dilation by the sum of the two radii) and every
 * station of every lattice candidate tests the n_discs centres (x, y) + o_d (cos theta, sin theta) against it -- a rectangle-aware
 * test for the price of n_discs bit tests.  n_discs = 0 restores the point test on the grid with the caller's inflation alone.  Needs the grid;
 * f1p_set_grid clears it.  Plans with a footprint run the mixed-precision schedule (round 5: the same prologue + candidate kernel pair as
 * point-footprint plans, at every batch size, with or without a clearance map); outputs are bit-identical to the all-fp64 kernel. */
int f1p_set_footprint(f1p_ctx* ctx, int32_t n_discs, const double* offsets, double radius);

/* TEST HOOK, read-only: one of the context's three bit-packed maps, unpacked on the host.  which = 0: the grid as uploaded
 * (f1p_set_grid), 1: the ACTIVE bitmap every collision test reads (the upload dilated by f1p_inflate_grid + f1p_set_footprint),
 * 2: the clearance map of the active bitmap the f32 filters use (built by the plans that want one).  cells: u8 [h][w] in the
 * image's row order (row 0 = top), 1 = bit set.  padding_all_set (nullable): 1 when every bit of the packed rows beyond column w
 * is set (the packing rule: beyond the right edge is occupied; also 1 when w is a multiple of 32), else 0.  clear_dist_cells
 * (nullable): the centre distance [cells] the current clearance map was built for, 0 when there is none or it is stale.
 * F1P_ESTATE without a grid, and for which = 2 while the clearance map is absent or stale; F1P_EINVAL for another `which` or a
 * NULL cells.  Synchronises the stream; changes nothing. */
int f1p_grid_debug_read(f1p_ctx* ctx, int32_t which, uint8_t* cells, double* clear_dist_cells, int32_t* padding_all_set);
/* TEST HOOK, read-only: the point test of the collision checks, one thread per point on the ACTIVE bitmap.  pts [E][2] (x, y) in
 * metres -> out [E] u8: 1 when the point's cell (f1p_set_grid's rule) is occupied, lies outside the image or a coordinate is not
 * finite, else 0.  E = 0 is a no-op. */
int f1p_grid_occupied_batch(f1p_ctx* ctx, const double* pts, int32_t E, uint8_t* out);

/* ------------------------------------------------------------------------------------------------
 * Leaf kernels of utils/utils.py, batched over E query points against the ctx waypoints.
 * ---------------------------------------------------------------------------------------------- */
/* nearest_point (utils/utils.py:37-67).  pts [E][2] -> proj [E][2], dist [E], t [E], idx [E] (segment index
 * in [0, n-2], first minimum wins).  Any output pointer may be NULL. */
int f1p_nearest_point_batch(f1p_ctx* ctx, const double* pts, int32_t E, double* proj, double* dist, double* t,
                            int32_t* idx);
/* intersect_point (utils/utils.py:69-151).  pts [E][2], start_t [E] (the `t` argument, i + t), one radius,
 * wrap flag -> first_p [E][2], first_i [E] (may be -1 in the wrap loop), first_t [E], found [E] (0 = None). */
int f1p_intersect_point_batch(f1p_ctx* ctx, const double* pts, const double* start_t, int32_t E, double radius,
                              int32_t wrap, double* first_p, int32_t* first_i, double* first_t, int32_t* found);

/* ------------------------------------------------------------------------------------------------
 * PurePursuitPlanner.plan (control/pure_pursuit/pure_pursuit.py:85-122) for E egos.
 * poses [E][3] = (x, y, theta).  Outputs: steer [E], speed [E] (the reference returns (steer, speed),
 * :122), near_idx [E] (nearest segment), la_idx [E] (look-ahead segment i2, may be -1; INT32_MIN when not
 * in the intersect branch), status [E] (F1P_ST_*).  near_idx / la_idx / status may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int f1p_pure_pursuit_batch(f1p_ctx* ctx, const double* poses, int32_t E, double lookahead, double wheelbase,
                           double max_reacquire, double* steer, double* speed, int32_t* near_idx,
                           int32_t* la_idx, int32_t* status);
int f1p_pure_pursuit_dev(f1p_ctx* ctx, const double* d_poses, int32_t E, double lookahead, double wheelbase,
                         double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near_idx,
                         int32_t* d_la_idx, int32_t* d_status);
/* Kernel form of f1p_pure_pursuit_*: egos per wave.  0 (default) = by batch size (1 below 8 192 egos, then 4 / 8 / 16 from 8 192 / 65 536 /
 * 262 144: a wave takes its egos one after the other through the 64-lane scans and runs plan()'s scalar part for all of them in one pass --
 * k_pure_pursuit16<G>, racelines of up to 4 097 waypoints), 1 = one ego per wave (k_pure_pursuit), 4 | 8 | 16 = that many.  Identical outputs
 * in every form (A/B timing; the tests compare them). */
int f1p_pure_pursuit_set_form(f1p_ctx* ctx, int32_t egos_per_wave);

/* ------------------------------------------------------------------------------------------------
 * SURVEY.md 8f rank 1 -- the two other waypoint trackers, batched on the same nearest-segment kernel.
 * StanleyPlanner.plan (control/stanley/stanley.py:114-139): states [E][4] = (x, y, theta, velocity) ->
 *   steer [E] = atan2(k_path * ef, v) + theta_e, speed [E] = waypoints[target, 2], near_idx [E] (nullable).
 * LQRPlanner.plan (control/lqr/lqr.py:156-210) with solve_lqr / update_matrix (utils/utils.py:167-239):
 *   err [E][2] carries (e_cog, theta_e) of the previous call (the planner's attributes, lqr.py:57-58) and is
 *   updated in place; q[4] = diag Q, r = R, max_iter / eps of the Riccati iteration; needs a curvature column.
 * ---------------------------------------------------------------------------------------------- */
int f1p_stanley_batch(f1p_ctx* ctx, const double* states, int32_t E, double wheelbase, double k_path, double* steer,
                      double* speed, int32_t* near_idx);
int f1p_lqr_batch(f1p_ctx* ctx, const double* states, double* err, int32_t E, double wheelbase, double timestep,
                  const double q[4], double r, int32_t max_iter, double eps, double* steer, double* speed,
                  int32_t* near_idx);

/* ------------------------------------------------------------------------------------------------
 * Track sets: every ego follows its own polyline.  The reference hands each planner its waypoints per call --
 * PurePursuitPlanner.plan(..., waypoints) (control/pure_pursuit/pure_pursuit.py:85), StanleyPlanner.plan
 * (control/stanley/stanley.py:114), LQRPlanner.plan (control/lqr/lqr.py:156), KMPCPlanner.plan(states, waypoints)
 * (control/kinematic_mpc/kinematic_mpc.py:115), STMPCPlanner.plan (control/dynamic_mpc/dynamic_mpc.py:133) -- so one planner
 * per vehicle can follow any line.  A track set holds K such
 * lines next to the ctx's raceline (the two are independent; f1p_set_waypoints does not touch the set, nor the reverse), and
 * the *_tracks calls take track_id [E] int32: ego e follows track track_id[e].  Each ego's outputs are bit-identical to the
 * single-raceline call on a ctx whose raceline is that ego's track.  An id outside [0, K) gives that ego NaN steer / speed
 * (NaN rows for the MPC reference), near_idx / idx -1, status F1P_ST_BAD_TRACK, and the call still succeeds; the other egos
 * are unaffected.  A *_tracks call without a track set returns F1P_ESTATE.
 * ---------------------------------------------------------------------------------------------- */
/* wp: row-major [row_offsets[K]][ncols] fp64, track k = rows [row_offsets[k], row_offsets[k+1]); columns as
 * f1p_set_waypoints_ex (col_psi / col_kappa < 0: none).  row_offsets[0] = 0, every track >= 2 rows, fewer than 2^31 rows in
 * all, headings finite within +-1e4 rad; otherwise F1P_EINVAL and the previous set stays in place.  A second call replaces
 * the set; K = 0 clears it (wp and row_offsets may then be NULL). */
int f1p_set_track_set(f1p_ctx* ctx, const double* wp, const int64_t* row_offsets, int32_t K, int32_t ncols, int32_t col_x,
                      int32_t col_y, int32_t col_v, int32_t col_psi, int32_t col_kappa);
/* nearest_point (utils/utils.py:37-67) of pts [E][2] on each ego's track: outputs as f1p_nearest_point_batch */
int f1p_nearest_point_tracks_batch(f1p_ctx* ctx, const double* pts, const int32_t* track_id, int32_t E, double* proj, double* dist,
                                   double* t, int32_t* idx);
/* PurePursuitPlanner.plan (pure_pursuit.py:85-122) on each ego's track: arguments and outputs as f1p_pure_pursuit_batch / _dev
 * (one ego per wave whatever f1p_pure_pursuit_set_form says) */
int f1p_pure_pursuit_tracks_batch(f1p_ctx* ctx, const double* poses, const int32_t* track_id, int32_t E, double lookahead,
                                  double wheelbase, double max_reacquire, double* steer, double* speed, int32_t* near_idx,
                                  int32_t* la_idx, int32_t* status);
int f1p_pure_pursuit_tracks_dev(f1p_ctx* ctx, const double* d_poses, const int32_t* d_track_id, int32_t E, double lookahead,
                                double wheelbase, double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near_idx,
                                int32_t* d_la_idx, int32_t* d_status);
/* StanleyPlanner.plan (stanley.py:114-139) on each ego's track (needs a heading column, else F1P_ESTATE) */
int f1p_stanley_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, double wheelbase, double k_path,
                             double* steer, double* speed, int32_t* near_idx);
/* LQRPlanner.plan (lqr.py:156-210) on each ego's track (needs heading and curvature columns, else F1P_ESTATE); err as
 * f1p_lqr_batch, left untouched for an ego with a bad track id */
int f1p_lqr_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, double* err, int32_t E, double wheelbase,
                         double timestep, const double q[4], double r, int32_t max_iter, double eps, double* steer, double* speed,
                         int32_t* near_idx);
/* calc_ref_trajectory_kinematic (kinematic_mpc.py:162-206) on each ego's track (cols x, y, v, psi; needs a heading column):
 * as f1p_kmpc_ref_batch, with f1p_kmpc_set_yaw_fixup honoured the same way (the fix-up acts on a per-ego view, never on the
 * stored tracks).  The _dev twin is asynchronous on device buffers, for f1p_kmpc_plan_dev / f1p_kmpc_qp_dev. */
int f1p_kmpc_ref_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, int32_t horizon, double dt,
                              double dl, double* ref);
int f1p_kmpc_ref_tracks_dev(f1p_ctx* ctx, const double* d_states, const int32_t* d_track_id, int32_t E, int32_t horizon, double dt,
                            double dl, double* d_ref);
/* calc_ref_trajectory (dynamic_mpc.py:195-233) on each ego's track: as f1p_stmpc_ref_batch (needs a heading column); with
 * (TK, DTK, dlk) STMPCPlanner's calc_ref_trajectory_kinematic (:237-276), rows 0, 1, 3, 4.  A bad id gives all 7 (T+1) entries NaN.
 * The _dev twin is asynchronous on device buffers, for f1p_stmpc_shoot_dev / f1p_stmpc_qp_dev. */
int f1p_stmpc_ref_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, int32_t horizon, double dt,
                               double dl, double* ref);
int f1p_stmpc_ref_tracks_dev(f1p_ctx* ctx, const double* d_states, const int32_t* d_track_id, int32_t E, int32_t horizon, double dt,
                             double dl, double* d_ref);
/* f1p_stmpc_qp_plan_tracks_batch, STMPCPlanner.plan's QP on each ego's track, is declared after f1p_stmpc_qp_plan_batch below (it
 * takes the dynamic-MPC structs). */

/* ------------------------------------------------------------------------------------------------
 * LatticePlanner.plan (planning/lattice_planner/lattice_planner.py:174-214) for E egos, one fused launch:
 * goal sampling (intent of sample_lookahead_square :223-260) -> G1 clothoid fit (pyclothoids
 * Clothoid.G1Hermite, :196) -> sample_traj at S stations (utils/utils.py:286-295) -> occupancy check
 * (map_collision stub, utils/utils.py:297-301) -> eval weighted cost (:130-156) -> select argmin
 * (:159-172) -> PurePursuitPlanner.plan on the winner (:208-212).
 *
 *   poses      [E][4]       (x, y, theta, velocity), map frame
 *   goals      [E][C][3]    optional host/device-supplied goals (x, y, theta) in the EGO frame, as the
 *                           G1Hermite(0,0,0, ...) call implies; NULL = sample on the device from
 *                           cfg.lookahead x cfg.width along the ctx waypoints
 *   prev_theta [E][S]       optional heading column of the previous plan's winner (similarity cost);
 *                           NULL = no previous path (term = 0)
 * Outputs (any may be NULL except steer/speed/best_idx; a candidate shard, cfg.cand_count > 0, only EVALUATES: it writes
 * best_idx, best_cost and near_idx, and the host-pointer wrapper rejects steer / speed / status / best_traj with F1P_EINVAL --
 * the global winner is emitted with f1p_lattice_emit_dev after the cross-rank argmin):
 *   steer, speed [E]; best_idx [E] (global candidate index, np.argmin first-minimum rule);
 *   best_cost [E]; status [E]; near_idx [E] (nearest raceline segment);
 *   best_traj [E][S][4] rows (x, y, theta, |kappa|) in the ego frame -- the third return value of plan();
 *   all_cost [E][C] and all_traj [E][C][S][4]: the materialised data flow of the reference (:194-201),
 *   needed by host-side Python cost callables; leave NULL for the fused path.
 * ---------------------------------------------------------------------------------------------- */
int f1p_lattice_plan_batch(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                           int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                           int32_t* best_idx, double* best_cost, int32_t* status, int32_t* near_idx,
                           double* best_traj, double* all_cost, double* all_traj);
int f1p_lattice_plan_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                         int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                         int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                         double* d_best_traj, double* d_all_cost, double* d_all_traj);
/* The same plan with the winner's trajectory as f32 rows [E][S][4] (x, y, theta, |kappa|): the fp64 rows of f1p_lattice_plan_*
 * rounded ONCE on the device, everything else unchanged (steer / speed / cost stay fp64, indices exact).  BASELINE's tolerance for
 * best_traj is 1e-4; a 4 m trajectory in f32 is good to 2.4e-7 m.  Half the bytes across PCIe: at 4096 egos x 50 stations the
 * trajectories are 3.3 MB instead of 6.6 MB of a 6.7 MB result (SURVEY 8b proposed float outputs).  Winner-only (no all_cost /
 * all_traj). */
int f1p_lattice_plan_batch_f32(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                               int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                               int32_t* best_idx, double* best_cost, int32_t* status, int32_t* near_idx, float* best_traj32);
int f1p_lattice_plan_dev_f32(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                             int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                             int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx, float* d_best_traj32);
/* Closed-loop mode.  The reference's fourth cost, get_similarity_cost (lattice_planner.py:287-296), compares a candidate's heading column
 * with the PREVIOUS plan's best trajectory, so a caller of the reference carries best_traj[:, 2] from one plan() to the next.  on = 1: the
 * context keeps the heading column of every plan's winners on the device ([E][S] fp64, two ctx-owned buffers used alternately, written by
 * the kernel that emits best_traj) and every following f1p_lattice_plan_* / f1p_lattice_step_* call of the same (E, S) that passes
 * prev_theta == NULL uses it as its prev_theta -- nothing crosses PCIe.  The first plan after (re)arming, or after the batch shape changed,
 * has no previous path (term = 0), like the reference's first call.  An explicit prev_theta still wins; a candidate shard
 * (cfg.cand_count > 0) reads the kept headings, f1p_lattice_emit_dev writes them.  on = 0: off (and forgotten).
 * f1p_lattice_closed_loop_state returns the device pointer / shape of the headings the NEXT plan would use (NULL / 0 when none). */
int f1p_lattice_set_closed_loop(f1p_ctx* ctx, int32_t on);
int f1p_lattice_closed_loop_state(f1p_ctx* ctx, const double** d_prev_theta, int32_t* E, int32_t* S);

/* One closed-loop control step for E egos -- what a simulator / vehicle fleet calls once per tick (the loop of
 * examples/control/pure_pursuit.py:35-58 with LatticePlanner.plan, lattice_planner.py:174-214, for E vehicles): poses [E][4] in,
 * steer [E], speed [E] and (nullable) status [E] out.  It always runs as a link of a closed loop: the previous STEP's headings
 * are the similarity term's previous path and never leave the device (round 5: the mode is scoped to the step -- a context whose caller never
 * called f1p_lattice_set_closed_loop(ctx, 1) keeps the chain between steps, and its f1p_lattice_plan_* calls neither read nor overwrite it); best_traj is NOT returned (keep_traj = 1 keeps the winners'
 * rows in HBM, f1p_lattice_fetch_traj copies them out on request: [E][S][4] fp64).  No copy is submitted in either direction: the
 * kernels read the poses from, and store the results into, page-locked host memory -- the caller's own arrays when they are
 * page-locked (f1p_host_alloc / hipHostRegister), a block of the context otherwise.  Device-sampled goals, whole egos
 * (cfg.cand_count == 0).  Outputs are those of f1p_lattice_plan_batch on the same chain, bit for bit. */
int f1p_lattice_step_batch(f1p_ctx* ctx, const double* poses, int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                           int32_t* status, int32_t keep_traj);
int f1p_lattice_fetch_traj(f1p_ctx* ctx, double* best_traj, int32_t E, int32_t S);

/* The lattice plan on a TRACK SET (f1p_set_track_set): ego e plans along track k = track_id[e], exactly as f1p_lattice_plan_* /
 * f1p_lattice_step_batch on a ctx whose raceline is track k (same map, footprint, clearance, cfg and prev_theta) -- nearest segment,
 * look-ahead goals and the speed command come from track k, near_idx is the row index within track k; every output bit for bit.
 * Arguments as the single-raceline calls plus track_id [E] int32 (d_track_id: device memory, asynchronous).  Every path of those
 * calls is taken (page-locked arrays, slices, pipeline, candidate slices, host goals -- which use the track for the nearest segment
 * and the speed only --, all_cost / all_traj, f1p_lattice_set_mode, the runtime audit); the step chains as f1p_lattice_step_batch.
 * An id outside [0, K) reads nothing of the set: NaN steer / speed / best_cost, best_idx and near_idx -1, status F1P_ST_BAD_TRACK,
 * zero rows and zero kept headings (its next plan with a valid id sees a zero previous path); the other egos are unaffected and the
 * call succeeds.  No track set, or device goals on a set without a heading column: F1P_ESTATE.  cfg.cand_count > 0 or a NULL
 * track_id with E > 0: F1P_EINVAL.  The ctx's raceline is not needed. */
int f1p_lattice_plan_tracks_batch(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta, const int32_t* track_id,
                                  int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                                  double* best_cost, int32_t* status, int32_t* near_idx, double* best_traj, double* all_cost,
                                  double* all_traj);
int f1p_lattice_plan_tracks_batch_f32(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                                      const int32_t* track_id, int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                                      int32_t* best_idx, double* best_cost, int32_t* status, int32_t* near_idx, float* best_traj32);
int f1p_lattice_plan_tracks_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                                const int32_t* d_track_id, int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                                int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                                double* d_best_traj, double* d_all_cost, double* d_all_traj);
int f1p_lattice_step_tracks_batch(f1p_ctx* ctx, const double* poses, const int32_t* track_id, int32_t E, const f1p_lattice_cfg* cfg,
                                  double* steer, double* speed, int32_t* status, int32_t keep_traj);

/* Evaluation schedule of f1p_lattice_plan_* (clothoid generator, winner-only outputs).
 *   mixed = 1 (default): every plan shape at every batch size (device- or host-supplied goals, clothoid or cubic candidates, point or
 *     oriented footprint, with or without a map; round 5) runs an f32 filter over the candidates (fit, cost bracket; lazily: stations,
 *     occupancy) that brackets each candidate's fp64 cost and classifies its collision status as certain / uncertain; only the
 *     candidates that can still be the minimum (typically 1-3 per ego) are re-evaluated by the fp64 arithmetic of the plain
 *     kernel, and the decision is taken on those fp64 costs -- every output is bit-identical to mixed = 0;
 *   mixed = 2: the same for any batch size, with the two-egos-per-wave prologue (k_lattice_prologue2) at any batch size too (mixed = 1 takes it
 *     from 3072 egos, where it is the faster one);  mixed = 0: all fp64 (with cfg.prune: branch and bound);
 *   mixed = 3: as 2 with the one-ego-per-wave prologue (k_lattice_prologue) at any batch size: identical outputs, kept for A/B timing and as
 *     the tests' second implementation.
 * d_cost32 [E][C] f32 and d_state [E][C] i32 (device pointers, nullable) receive the filter's costs and states
 * (0 free, 1 hit, 2 unsure, 3 infeasible) of the following launches: the hook the tests calibrate the margins with. */
int f1p_lattice_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_state);

/* Workgroups per ego of the single-kernel schedules: 0 = automatic (with fewer egos than half the CUs and more than 256
 * candidates -- BASELINE configs[1], one ego x 512 candidates -- each workgroup evaluates a slice of 256 candidates and the last
 * one to finish merges the partial winners, re-emits and tracks: no second launch); n > 0 forces n slices (tests, A/B runs). */
int f1p_lattice_set_split(f1p_ctx* ctx, int32_t groups);

/* Moving obstacles on the lattice planner's candidates.
 * Inputs, per ego e:
 *   - up to F1P_LATTICE_MAX_OBS = 16 slots obs[e][m] = (x, y, vx, vy, r): fp64, map frame, constant velocity;
 *   - a slot with !(r >= 0) is empty; empty slots may sit anywhere;
 *   - the caller folds the vehicle's own radius into r; with an oriented footprint installed, that is the footprint's disc radius;
 *   - a pace pace[e] in s/m, meaning seconds per metre of path.
 * Time of a station: station j has the time tau_j = s_j * pace[e].
 *   - clothoid: s_j = (double)j * ds, with ds exactly as station_loop forms it (L / (double)max(S - 1, 1));
 *   - cubic: s_j is the chord sum that station_loop accumulates in len up to station j, with 0 at j = 0;
 *   - pace = 0 makes every disc a parked one.
 * Tested points: exactly the points the occupancy test tests: every station j = 0 .. S-1, as the station point (qx, qy) in the ego
 * frame; with an oriented footprint (and the occupancy test running: a grid loaded, cfg.check_collision on) the footprint's disc centres instead.
 * Slot transform, once per ego and live slot, in fp64 and in this order, with (ct, st) the cos / sin of the pose heading the kernels already hold:
 *   dx0 = x - px; dy0 = y - py
 *   ax = ct*dx0 + st*dy0; ay = ct*dy0 - st*dx0
 *   ux = ct*vx + st*vy; uy = ct*vy - st*vx
 *   rr = r*r
 * Point test, per tested point and live slot:
 *   cx = ax + ux*tau; cy = ay + uy*tau
 *   dx = qx - cx; dy = qy - cy; d2 = dx*dx + dy*dy
 *   the point is blocked when !(d2 > rr)
 * -- touching blocks; a NaN anywhere blocks: a NaN pace or slot value blocks every candidate of that ego; no contraction, as everywhere
 * else in the library (-ffp-contract=off).
 * Decision: a candidate with a blocked point costs +inf, exactly like one through an occupied cell; the decision, all_cost,
 * F1P_ST_ALL_BLOCKED and the all-blocked outputs are the occupancy test's.  The disc test applies with or without a grid, and with
 * cfg.check_collision on or off.  An ego without a live slot gets the bits of a plan without obstacles.
 * f1p_lattice_set_obstacles copies both arrays into buffers of the context on its stream; obs == NULL or M == 0 clears.
 * f1p_lattice_set_obstacles_dev BORROWS device arrays: the caller keeps them alive and may rewrite them in place between plans (in
 * stream order).  The obstacles stay until the next set or clear and apply to f1p_lattice_plan_batch / _dev / _batch_f32 / _dev_f32, the
 * four f1p_lattice_plan_tracks_*, f1p_lattice_step_batch and f1p_lattice_step_tracks_batch, with and without all_cost / all_traj (a blocked
 * candidate's all_cost is +inf, its rows are unchanged), under every f1p_lattice_set_mode (every mode equals mode 0 bit for bit), slices
 * and pipelined chunks (the per-ego arrays are indexed by the absolute ego), the closed-loop chain, cfg.prune and the runtime audit.
 * Errors, nothing launched: M outside [1, 16] or a NULL pace: F1P_EINVAL; a plan whose E differs from the E the obstacles were set for:
 * F1P_ESTATE; while obstacles are set, a candidate shard (cfg.cand_count > 0), f1p_lattice_emit_dev and f1p_lattice_set_split(> 0)
 * (and setting obstacles while a split is forced): F1P_ESTATE.  Not covered: a MultiContext's sharded plans. */
#define F1P_LATTICE_MAX_OBS 16
int f1p_lattice_set_obstacles(f1p_ctx* ctx, const double* obs, const double* pace, int32_t E, int32_t M);
int f1p_lattice_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, const double* d_pace, int32_t E, int32_t M);

/* Occupancy test of the f32 filter (mixed schedule).  stations_each_side = r > 0 (default 2; a smaller r is taken when the clearance zone of r would not fit the ego's tile): the filter
 * looks up one station in 2 r + 1 in a CLEARANCE map of the active bitmap (cells whose centre is within
 * r * ds_cap + (sqrt 2 + 1) cells of an occupied or off-map cell, ds_cap = 1.2 * hypot(max look-ahead, max width) / (S - 1);
 * built on the device at the first plan and whenever the bitmap changes): a tested station in a clear cell proves the r
 * stations before and after it collision-free, anything else is decided by the fp64 kernels on the real bitmap, so every
 * output stays bit-identical.  r = 0: no clearance map -- every station of a looked-at candidate against the bitmap itself with a
 * boundary band.  Range 0..2. */
int f1p_lattice_set_clearance(f1p_ctx* ctx, int32_t stations_each_side);

/* Runtime audit of the mixed-precision schedule.  every_n > 0: every every_n-th f1p_lattice_plan_* call that runs the mixed
 * schedule (device-sampled goals, full plan) is followed, on the same stream, by the all-fp64 exhaustive kernel (cfg.prune = 0,
 * f1p_lattice_set_mode 0's kernel) on a window of n_egos consecutive egos whose position moves with every audited plan, and by a
 * comparison of EVERY output of those egos -- steer, speed, best_idx, best_cost, status, near_idx, best_traj (fp64 rows bit for bit,
 * f32 rows against the fp64 rows rounded once).  f1p_lattice_audit_read returns {plans audited, egos audited, egos with any
 * mismatch} since the last reset (synchronises the stream).  The mixed schedule's exactness rests on error margins that are
 * derived in DESIGN.md and measured in the tests; this is the belt to those braces: a production caller can keep every_n = 64
 * (a 64-ego window costs ~40 us, i.e. < 1 us per plan amortised) and alarm on a non-zero third counter.  every_n = 0: off. */
int f1p_lattice_set_audit(f1p_ctx* ctx, int32_t every_n, int32_t n_egos);
int f1p_lattice_audit_read(f1p_ctx* ctx, uint64_t out[3], int32_t reset);
/* TEST HOOK, not for production: replaces the f32 filter's cost margins (|cost64 - cost32| <= margin_rel * sum|terms| + margin_abs)
 * while enable != 0.  Margins below the filter's real error (e.g. negative ones) make the mixed schedule return WRONG winners:
 * that is what tests/test_gpu_audit.py uses it for -- to show that the audit above fires.  enable = 0 restores the defaults. */
int f1p_lattice_debug_margins(f1p_ctx* ctx, int32_t enable, float margin_rel, float margin_abs);
/* TEST / MEASUREMENT HOOK: entries_per_ego [E] (host) <- how many candidates of each ego the LAST mixed-schedule plan of E egos handed to the
 * fp64 refinement (the f32 winner plus whatever the brackets could not rank; synchronises the stream). */
int f1p_lattice_debug_queue(f1p_ctx* ctx, int32_t* entries_per_ego, int32_t E);
/* TEST HOOK: d_bound [E][C] f32 (device pointer, nullable) receives every candidate's A-PRIORI cost error bound of the following
 * mixed plans (the running bound of LABNOTES.md 5c that widens the candidate's bracket when it exceeds the calibrated margin); the tests
 * check bound >= |cost32 - cost64| candidate by candidate. */
int f1p_lattice_debug_bound(f1p_ctx* ctx, float* d_bound);
/* TEST HOOK: the slack [m] of the look-ahead filters (chunk-box reach, f32 bracket, surely_none) that a mixed plan with this configuration gets
 * on the context's raceline (tracks = 0) or track set (tracks != 0): 1e-4 / 1e-4f on an ordinary map, the rounding bound of the reference's
 * quadratic where that is larger (lookahead_slack, k_lattice_mixed.hip).  Host arithmetic only; nothing is launched. */
int f1p_lattice_debug_slack(f1p_ctx* ctx, const f1p_lattice_cfg* cfg, int32_t tracks, double* slack, float* slack_f);
/* Dispatch order of the mixed schedule's candidate kernel (round 5).  1 (default): every plan of >= 1024 egos leaves one flag per ego -- its
 * cheapest candidates collided, so its workgroup took the long path -- and the next plan of the same batch size starts those egos' workgroups
 * first, where their longer lifetime overlaps the others instead of ending the kernel (a control loop meets the same obstacle in consecutive
 * plans).  0: ego order.  Outputs are identical either way; the order only moves time.  Applies to UNPIPELINED plans only: a plan cut into chunks of
 * egos (f1p_lattice_set_pipeline with chunks > 1) runs every chunk in ego order, and plans profiled per kernel (f1p_lattice_profile) are unpipelined. */
int f1p_lattice_set_order(f1p_ctx* ctx, int32_t heavy_first);
/* MEASUREMENT HOOK (round 5): d_pass [E][4] i32 (device pointer, nullable; the caller zeroes it) receives, per ego of the following mixed
 * plans, what the candidate kernel's LAZY station pass looked at: [0] candidates whose positions were integrated and looked up (certain
 * hits included -- f1p_lattice_debug_queue only counts what reaches the fp64 refinement), [1] passes that ran lane-per-candidate,
 * [2] rounds of the pass, [3] candidates that took the SECOND look (every station against the real bitmap).  The pass itself is unchanged (bench.py's scene_sweep reads it). */
int f1p_lattice_debug_pass(f1p_ctx* ctx, int32_t* d_pass);

/* Pipelining of one mixed-schedule plan: the ego batch is cut into `chunks` contiguous chunks whose kernels (prologue, candidate
 * filter, fp64 refinement, selection) run on two internal streams, the second one stage behind the first, so one chunk's
 * latency-bound kernels overlap the other's VALU-bound filter.  The caller's stream is joined before and after: the call keeps
 * its in-order semantics and every output is unchanged (egos are independent).  0 = automatic (currently 1: measured slower than
 * unpipelined on one MI355X -- the candidate kernel fills every wave slot and each cross-stream edge costs ~10 us), 1 = off, up to 8. */
int f1p_lattice_set_pipeline(f1p_ctx* ctx, int32_t chunks);

/* Per-kernel timing of the mixed schedule: enable = 1 records HIP events on the ctx stream around the kernels of every following
 * plan (which then runs unpipelined); kernel_ms (nullable) receives the four durations of the LAST profiled plan (synchronises
 * on it): [0] k_lattice_prologue (0 when the one-kernel filter ran), [1] the f32 candidate filter, [2] k_lattice_refine,
 * [3] k_lattice_select.  bench.py takes the dominant kernel's duration for `roofline` from here.  (Round 3: four values, the
 * prologue is its own kernel.) */
int f1p_lattice_profile(f1p_ctx* ctx, int32_t enable, float kernel_ms[4]);

/* Re-generate candidate `cand_idx[e]` of each ego and track it: the "emit" half of plan(), used after a
 * cross-rank argmin when one ego's candidates are sharded over several GPUs. */
int f1p_lattice_emit_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, int32_t E,
                         const f1p_lattice_cfg* cfg, const int32_t* d_cand_idx, const double* d_cand_cost,
                         double* d_steer, double* d_speed, int32_t* d_status, int32_t* d_near_idx,
                         double* d_best_traj);

/* Clothoid leaf: G1 Hermite fit from (0,0,0) to each goal (x, y, theta) -- what
 * pyclothoids.Clothoid.G1Hermite(0,0,0,x,y,theta) returns (lattice_planner.py:196).
 * goals [n][3] -> kappa0 [n], dkappa [n], length [n], ok [n] (0 = Newton did not converge / degenerate).
 * Domain: a chord r = hypot(x, y) <= 1e-12 or a value that is not finite is rejected (ok = 0, zero parameters) and wherever ok = 1
 * all three parameters are finite; pinned to a 50-digit reference for r = 1.1e-12 .. 1e150 and any finite theta (reduced by whole multiples of
 * the double 2 pi; straight behind the ego the sign of a zero y picks the side).  From r ~ 1.3e154 length^2 overflows and dkappa is 0. */
int f1p_clothoid_g1_batch(f1p_ctx* ctx, const double* goals, int32_t n, double* kappa0, double* dkappa,
                          double* length, int32_t* ok);

/* sample_traj (utils/utils.py:286-295) for n clothoids given by their parameters: params [n][3] = (kappa0, dkappa, length) in
 * each clothoid's own start frame (start pose (0, 0, 0)) -> rows [n][npts][4] = (X(s_i), Y(s_i), Theta(s_i), |kappa(s_i)|) at
 * s_i = i * length / max(npts - 1, 1), the arithmetic of the planner's station loop.  That arithmetic holds up to 4096 pieces per
 * station interval (ceil(max|kappa| ds / 0.3) and ceil(2.5 ds sqrt|dkappa|), ds = length / max(npts - 1, 1)): a clothoid beyond that, or
 * with a parameter that is not finite, gets NaN in all its rows; the others are unaffected and the call succeeds.  A G1 fit stays below 60. */
int f1p_clothoid_sample_batch(f1p_ctx* ctx, const double* params, int32_t n, int32_t npts, double* rows);

/* ------------------------------------------------------------------------------------------------
 * Kinematic MPC by random shooting for E egos: R open-loop rollouts of
 * predict_motion_kinematic / update_state_kinematic (control/kinematic_mpc/kinematic_mpc.py:208-243),
 * the objective of :324-334 evaluated on the nonlinear rollout, argmin, output map of :506-508.
 *   x0       [E][4]          (x, y, v, yaw)                       fp64
 *   ref      [E][4][T+1]     calc_ref_trajectory_kinematic output (:162-206), rows x, y, v, yaw   fp64
 *   controls [E][T][2][R]    f32, (accel, steer) candidates, rollout index fastest (coalesced).  +-inf is clamped to the bound.  A NaN
 *                            stays a NaN through the bounds: that rollout's cost is NaN and, by np.argmin's rule, the first such rollout of
 *                            an ego wins (best_cost NaN) -- in both evaluation modes: the f32 filter hands a rollout with a NaN control
 *                            to the fp64 decision.  The same holds for generated controls: f1p_kmpc_warm_set / f1p_stmpc_warm_set note a
 *                            non-finite entry, and until the next set / reset the generated plans are evaluated in fp64 throughout
 *                            (non-finite sigmas are rejected with F1P_EINVAL).
 * Outputs: steer [E] = delta_0 of the winner, speed [E] = v + a_0*DTK, best_idx [E], best_cost [E],
 *   best_seq [E][T][2] (the winner's applied accel/steer after bound projection; may be NULL).
 * ---------------------------------------------------------------------------------------------- */
int f1p_kmpc_shoot_batch(f1p_ctx* ctx, const double* x0, const double* ref, const float* controls, int32_t E,
                         const f1p_kmpc_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                         double* best_cost, double* best_seq);
int f1p_kmpc_shoot_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, int32_t E,
                       const f1p_kmpc_cfg* cfg, double* d_steer, double* d_speed, int32_t* d_best_idx,
                       double* d_best_cost, double* d_best_seq);
/* predict_motion_kinematic (:208-221) for E egos: open-loop rollout of update_state_kinematic (:223-243).
 * x0 [E][4], oa [E][T], od [E][T] (fp64, used as given: only the steer clamp inside the step applies)
 * -> path [E][4][T+1], rows x, y, v, yaw; column 0 is x0. */
int f1p_kmpc_predict_batch(f1p_ctx* ctx, const double* x0, const double* oa, const double* od, int32_t E,
                           const f1p_kmpc_cfg* cfg, double* path);
/* Evaluation mode of f1p_kmpc_shoot_*: mixed = 1 (default): every rollout is ranked by an f32 filter that streams the
 * controls at HBM speed, the rollouts within a safety margin of the f32 minimum are re-evaluated in fp64 and the decision is
 * taken on those fp64 costs (identical best_idx / best_cost to the plain fp64 evaluation); mixed = 0: plain fp64.
 * d_cost32 [E][R] f32 and d_n_refined [E] i32 (both nullable, device pointers) receive the filter costs and the size of the
 * refined set (-1 = fp64 fallback) of the following launches -- the hook the parity tests use to measure the filter error. */
int f1p_kmpc_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_n_refined);
/* calc_ref_trajectory_kinematic (:162-206) for E egos against the ctx waypoints (cols x, y, v, psi):
 * states [E][4] = (x, y, v, yaw) -> ref [E][4][T+1].  The reference's in-place fix-up of cyaw (:198-203) is
 * applied to a per-ego view, never to the stored waypoints. */
int f1p_kmpc_ref_batch(f1p_ctx* ctx, const double* states, int32_t E, int32_t horizon, double dt, double dl,
                       double* ref);
/* fill controls [E][T][2][R] f32 on the device from a counter-based generator (seeded, reproducible):
 * accel ~ clip(N(0, sigma_a), +-max_accel), steer ~ clip(N(0, sigma_d), +-max_steer) */
int f1p_kmpc_sample_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_kmpc_cfg* cfg,
                                 uint64_t seed, double sigma_accel, double sigma_steer);

/* ------------------------------------------------------------------------------------------------
 * Shooting MPC with the controls GENERATED IN THE KERNEL and the warm start resident on the device: what
 * KMPCPlanner.plan does per call (kinematic_mpc.py:115-160, 477-508) with the QP replaced by sampling -- reference
 * extraction (:162-206), R candidate sequences around the previous solution shifted by one step (the reference's warm start
 * self.oa / self.odelta_v, :108-110, :491-498), rollout + objective + bounds, argmin, output map, new warm start.
 * Nothing per-rollout exists in memory: control (rollout r, step t) of ego e is a pure function of (seed, call, e, r, t):
 *   Philox4x32-10, counter = (t / 2, r, e, call), key = seed  ->  four 32-bit words = (accel, steer) of steps 2 (t/2), 2 (t/2) + 1;
 *   accel = fma(sigma_accel, z_a, warm_a[t]),  steer = fma(sigma_steer, z_d, warm_d[t])   in f32, where z = (sum of the word's 4
 *   bytes - 510) / 147.80054 is a standardised Irwin-Hall variate (bounded near-normal, integer arithmetic => bit-identical to the
 *   CPU restatement oracle/f1p_oracle.c:orc_kmpc_gen_controls); rollout 0 = the warm start itself, rollout 1 = all zero.
 * The bounds are applied by the rollout's projection exactly as for streamed controls, so
 *   f1p_kmpc_gen_controls_dev + f1p_kmpc_shoot_dev  ==  f1p_kmpc_plan_dev   bit for bit (tests/test_gpu_kmpc_gen.py).
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_kmpc_sampler {
    uint64_t seed;           /* Philox key                                                                          */
    uint32_t call;           /* plan counter (counter word 3): the caller increments it every plan                  */
    int32_t use_warm;        /* 1: sample around the ctx's warm start when it holds one for this (E, T); 0: around 0 */
    double sigma_accel;      /* std of the acceleration perturbation [m/s^2]                                        */
    double sigma_steer;      /* std of the steering perturbation [rad]                                              */
} f1p_kmpc_sampler;
/* x0 [E][4] = (x, y, v, yaw) HOST -> reference from the ctx waypoints (cols x, y, v, psi; dl = mpc_config.dlk) -> plan.
 * Outputs as f1p_kmpc_shoot_batch (best_cost / best_seq nullable).  Updates the ctx's warm start ([E][T][2] f32, device). */
int f1p_kmpc_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_kmpc_cfg* cfg, double dl,
                        const f1p_kmpc_sampler* smp, double* steer, double* speed, int32_t* best_idx, double* best_cost,
                        double* best_seq);
/* the same on device buffers with the reference trajectories given (d_ref [E][4][T+1]); asynchronous on the ctx stream */
int f1p_kmpc_plan_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, int32_t E, const f1p_kmpc_cfg* cfg,
                      const f1p_kmpc_sampler* smp, double* d_steer, double* d_speed, int32_t* d_best_idx,
                      double* d_best_cost, double* d_best_seq);
/* materialise the generated controls as the f32 [E][T][2][R] buffer of f1p_kmpc_shoot_dev (around the ctx's current warm
 * start when smp->use_warm and one is held): the parity hook "generated == streamed" */
int f1p_kmpc_gen_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_kmpc_cfg* cfg,
                              const f1p_kmpc_sampler* smp);
/* warm start of the ctx: forget it / read it back / install one (warm [E][T][2] f32 host = (accel, steer) per step) */
int f1p_kmpc_warm_reset(f1p_ctx* ctx);
int f1p_kmpc_warm_get(f1p_ctx* ctx, float* warm, int32_t E, int32_t T);
int f1p_kmpc_warm_set(f1p_ctx* ctx, const float* warm, int32_t E, int32_t T);
/* workgroups per ego of f1p_kmpc_plan_*: 0 = default (one: measured fastest at every batch size since the refinement and the
 * re-emission run with the time steps across lanes); > 0 forces the count -- each workgroup filters a slice of the rollouts, the
 * last one to finish reduces (tests, A/B runs) */
int f1p_kmpc_set_groups(f1p_ctx* ctx, int32_t groups);
/* Occupancy test on the rollouts of the shooting solver.
 * on = 0 (default): rollouts are not tested against the grid.  on = 1: a rollout of f1p_kmpc_plan_* / f1p_kmpc_shoot_* whose
 * tested points touch an occupied cell costs +inf.  n_sub in [1, 16]: points tested per time step.
 * Tested points: with p_0 .. p_T the states of the APPLIED sequence (bounds and rate limit) under update_state_kinematic, for
 * t = 0 .. T-1 and j = 1 .. n_sub the point p_t + (p_{t+1} - p_t) * ((double)j / (double)n_sub), per coordinate in fp64 in that
 * order; j = n_sub is p_{t+1} itself; p_0, the vehicle's present position, is not tested.
 * Cell rule: the lattice's, on the ACTIVE bitmap -- f1p_inflate_grid(r) makes it a disc test of radius r; a point outside the
 * image or a non-finite coordinate is occupied.
 * Decision: first minimum by rollout index over the unblocked rollouts (NaN costs as without the test).  Every rollout
 * blocked: best_idx = -1, best_cost = +inf, steer = 0, speed = 0, best_seq all zero, and the ego's warm-start row is set to zero.
 * f1p_kmpc_plan_* in the mixed mode runs an f32 filter that only decides what cannot win; outputs are bit-identical to mode 0.
 * f1p_kmpc_shoot_* (streamed controls) with the test on are evaluated in plain fp64 WHATEVER f1p_kmpc_set_mode says; with the
 * same controls they equal f1p_kmpc_plan_dev bit for bit (f1p_kmpc_gen_controls_dev).
 * With the test on, the entry points above return an error and launch nothing when no grid is loaded (F1P_ESTATE), when an
 * oriented footprint is installed (f1p_set_footprint with n_discs > 0: this is a point / disc test, use f1p_inflate_grid;
 * F1P_ESTATE) or when f1p_kmpc_set_groups(> 0) is in force (F1P_ESTATE).  n_sub outside [1, 16]: F1P_EINVAL, nothing changes.
 * Not covered: f1p_kmpc_qp_* (the QP has no rollouts to test; the grid is not among its constraints).  f1p_stmpc_* has a switch of its
 * own, f1p_stmpc_set_collision; this one does not reach it. */
int f1p_kmpc_set_collision(f1p_ctx* ctx, int32_t on, int32_t n_sub);
/* Moving obstacles on the rollouts of the shooting solver: per ego up to F1P_KMPC_MAX_OBS discs at constant
 * velocity, obs [E][M][5] fp64 rows (x, y, vx, vy, r) in the map frame.  A slot with !(r >= 0) -- r negative or NaN -- is EMPTY;
 * empty slots may sit anywhere.  The caller folds the ego's own radius into r (a point-against-disc test, like f1p_inflate_grid).
 * Tested points: f1p_kmpc_set_collision's, with its n_sub (the context keeps the number while `on` is 0; default 1).  The point of
 * step t at f = (double)j / (double)n_sub has the time tau = ((double)t + f) * dt; against a live slot, in fp64 and in this order,
 *   cx = x + vx * tau; cy = y + vy * tau; dx = Px - cx; dy = Py - cy; d2 = dx*dx + dy*dy;   blocked when !(d2 > r*r)
 * -- touching blocks, a NaN anywhere blocks.  A rollout is blocked when a tested point is blocked by a live slot, or by the grid
 * while f1p_kmpc_set_collision is on as well; the decision, the NaN-cost rule and the all-blocked outputs are that test's.  An
 * ego without a live slot gets the bits of a plan without obstacles.
 * f1p_kmpc_set_obstacles copies the array into a buffer of the context on its stream; obs == NULL or M == 0 clears.
 * f1p_kmpc_set_obstacles_dev BORROWS a device array: the caller keeps it alive and may rewrite it in place between plans (in
 * stream order).  The obstacles stay until the next set or clear and apply to f1p_kmpc_plan_batch / _dev and
 * f1p_kmpc_shoot_batch / _dev (raceline and track-set references alike), with or without a grid; the streamed entry points are
 * then evaluated in plain fp64 whatever the mode and equal f1p_kmpc_plan_dev bit for bit.
 * Errors, nothing launched: M outside [1, 16]: F1P_EINVAL; a plan whose E is not the E the obstacles were set for: F1P_ESTATE;
 * f1p_kmpc_set_groups(> 0) while obstacles are set (and setting obstacles while groups are forced): F1P_ESTATE.
 * f1p_kmpc_qp_plan_batch / f1p_kmpc_qp_dev take the same discs as soft half-plane rows of the QP while f1p_kmpc_qp_set_avoid is on
 * (below), and ignore them while it is off.
 * Not covered: f1p_stmpc_* (f1p_stmpc_set_obstacles is its own) and a MultiContext's sharded plans. */
#define F1P_KMPC_MAX_OBS 16
int f1p_kmpc_set_obstacles(f1p_ctx* ctx, const double* obs, int32_t E, int32_t M);
int f1p_kmpc_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, int32_t E, int32_t M);
/* The reference extraction's heading fix-up (calc_ref_trajectory_kinematic, kinematic_mpc.py:198-203: course headings more than
 * 4.5 rad from the vehicle's are folded by abs(. -+ 2 pi), IN PLACE and persistently on the caller's array).  on = 1 (default):
 * applied per ego to the gathered values, the course array is never modified (batches of egos with different headings).
 * on = 0: the course heading is used as uploaded -- for a caller that maintains the array itself exactly like the reference
 * (the single-vehicle KMPCPlanner class does, so that repeated plan() calls see the reference's persistent state). */
int f1p_kmpc_set_yaw_fixup(f1p_ctx* ctx, int32_t on);

/* ------------------------------------------------------------------------------------------------
 * Kinematic MPC as the reference solves it: the linearised QP of control/kinematic_mpc/kinematic_mpc.py, batched, fp64
 * (csrc/k_kmpc_qp.hip; DESIGN.md "The linearised QP").  Per ego:
 *   linearisation point (linear_mpc_control_kinematic :452-475): rows v, yaw of predict_motion_kinematic(x0, oa_prev, od_prev)
 *     (:208-243) -- the previous solution NOT shifted; zeros when NULL (the first call, after a reset);
 *   model (get_kinematic_model_matrix :245-278) at (v_t, phi_t, delta = 0): A[3][2] = 0, B[3][1] = DTK v / WB, C[3] = 0;
 *   problem (mpc_prob_init_kinematic :283-405):  min  sum_t u_t' Rk u_t + sum_{t<=T} (x_t - ref_t)' Q (x_t - ref_t) (Qfk at T)
 *     + sum_{t<T-1} (u_{t+1} - u_t)' Rdk (u_{t+1} - u_t)  s.t.  x_{t+1} = A_t x_t + B_t u_t + C_t, x_0 = x0, |a_t| <= MAX_ACCEL,
 *     |delta_t| <= MAX_STEER, |delta_{t+1} - delta_t| <= MAX_DSTEER DTK, MIN_SPEED <= v_t <= MAX_SPEED (t = 0..T);
 *     diagonal weights only (cfg q, qf, r, rd); r > 0 makes it strictly convex: one optimum;
 *   output map (:500-505): steer = delta_0, speed = v0 + a_0 DTK.
 * Feasible iff MIN_SPEED <= v0 <= MAX_SPEED (then a = delta = 0 is feasible; otherwise the t = 0 speed bound cannot hold).
 * Solver: primal-dual interior point (Mehrotra predictor-corrector) on the condensed problem (2T inputs), stopping when the scaled
 * KKT residuals and the duality gap are below opts->tol, or after opts->max_iter iterations (an ego whose Newton matrix stops being
 * numerically positive definite first counts as solved when its gap is below tol (1 + |objective|)).  2 <= horizon <= 32 (else
 * F1P_EINVAL).
 *   x0 [E][4] (x, y, v, yaw); ref [E][4][T+1] (f1p_kmpc_ref_batch); oa_prev, od_prev [E][T] (nullable: zeros)
 * Outputs: steer, speed [E]; status [E]: 0 solved, 1 infeasible, 2 not converged (the last iterate, like cvxpy's OPTIMAL_INACCURATE),
 *   3 non-finite input; statuses 1 and 3 give NaN in every output.  Nullable: u [E][T][2] (accel, steer), xk [E][4][T+1] (the
 *   states of the linear model), obj [E] (the value cvxpy reports, the constant t = 0 term included), iters [E], and
 *   duals [E][8T-2]: the multipliers of  a_t <= MAX_ACCEL (T), -a_t <= MAX_ACCEL (T), delta_t <= MAX_STEER (T), -delta_t <= MAX_STEER (T),
 *   delta_{t+1} - delta_t <= MAX_DSTEER DTK (T-1), its negation (T-1), v_t <= MAX_SPEED for t = 1..T (T), -v_t <= -MIN_SPEED (T).
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_kmpc_qp_opts {
    int32_t max_iter;        /* interior-point iterations at most (50)                                              */
    int32_t pad;
    double tol;              /* stop when the scaled KKT residuals and the gap are below it (1e-10)                  */
} f1p_kmpc_qp_opts;
void f1p_kmpc_qp_opts_default(f1p_kmpc_qp_opts* opts);
int f1p_kmpc_qp_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                      const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status, double* u,
                      double* xk, double* obj, double* duals, int32_t* iters);
/* the same on device buffers; asynchronous on the ctx stream */
int f1p_kmpc_qp_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                    const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* d_steer, double* d_speed, int32_t* d_status,
                    double* d_u, double* d_xk, double* d_obj, double* d_duals, int32_t* d_iters);
/* What KMPCPlanner.plan does per call with the QP solver (MPC_Control_kinematic :477-508) for E egos in one call: reference extraction
 * (:162-206) from the ctx waypoints (dl = mpc_config.dlk), linearisation about the ctx's QP warm start, solve, output map.  The warm start
 * is the previous call's solution u [E][T][2] fp64 (self.oa / self.odelta_v, :490-498), kept on the device and keyed by (E, T) like the
 * shooting one (separate from it); statuses 1 and 3 reset an ego's to zeros (the reference's None).  u, obj nullable. */
int f1p_kmpc_qp_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_kmpc_cfg* cfg, double dl, const f1p_kmpc_qp_opts* opts,
                           double* steer, double* speed, int32_t* status, double* u, double* obj);
/* the QP warm start: forget it / read it back / install one (warm [E][T][2] fp64 host) */
int f1p_kmpc_qp_warm_reset(f1p_ctx* ctx);
int f1p_kmpc_qp_warm_get(f1p_ctx* ctx, double* warm, int32_t E, int32_t T);
int f1p_kmpc_qp_warm_set(f1p_ctx* ctx, const double* warm, int32_t E, int32_t T);
/* egos per wave of the QP kernel at T <= 8: 0 = default, 1 or 4 forces it (timing runs; longer horizons always take one per wave) */
int f1p_kmpc_qp_set_pack(f1p_ctx* ctx, int32_t egos_per_wave);

/* Moving-disc avoidance in the QP: f1p_kmpc_set_obstacles' discs as SOFT, LINEARISED half-plane rows.  An avoidance
 * term, not a guarantee: the rows are linearised about the previous solution's path and softened by a slack; margin is the knob.
 * The problem of f1p_kmpc_qp_* is kept -- the same u, linearisation path and 8T-2 rows -- and gains
 *   one slack eps as input number 2T (n = 2T + 1): cost rho eps^2 + lin eps, row -eps <= 0;
 *   at most two rows per step t = 1..T.  pbar_t: the position of the linearisation path (predict_motion_kinematic of the previous
 *     solution) at step t.  A live slot (r >= 0) is predicted at tau = (double)t * dt: c = (x + vx tau, y + vy tau), d = pbar_t - c,
 *     dist = sqrt(dx^2 + dy^2), clear = dist - r.  The two live slots with the smallest clear are taken, ties to the lower slot;
 *     each gives the normal n = d / dist (dist < 1e-9: n = -(cos psibar_t, sin psibar_t), stay behind it) and, with x_t = S(t) u + s(t)
 *     the linear model's state, the row   -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - (r + margin).
 * An ego without a live slot has no such row and keeps eps and -eps <= 0.  Always feasible when f1p_kmpc_qp_* is (status 1 as there);
 * a live slot with a non-finite number: status 3.  2 <= horizon <= 31 (else F1P_EINVAL).  The warm start stays u [E][T][2]; eps is not
 * carried.  obj includes rho eps^2 + lin eps.
 * f1p_kmpc_qp_avoid_batch / _dev: f1p_kmpc_qp_batch / _dev with obs [E][M][5] (M in 1..16) and avoid (NULL: the defaults; `on` is not
 *   read), and the nullable outputs eps [E]; planes [E][T][2][4] = (n_x, n_y, right-hand side, slot as a double; slot -1 and zeros for
 *   an absent row); avoid_duals [E][2T+1]: the multipliers of the 2T avoidance rows in step order (0 for an absent row), then of
 *   -eps <= 0.  duals [E][8T-2] keeps its layout.  Statuses 1 and 3: NaN in all of them.
 * f1p_kmpc_qp_set_avoid: NULL or on = 0 turns it off (the default).  While on, f1p_kmpc_qp_plan_batch and f1p_kmpc_qp_dev solve this
 *   problem with the discs held by f1p_kmpc_set_obstacles[_dev] (none held: no avoidance rows); a plan whose E is not the E the
 *   obstacles were set for: F1P_ESTATE; horizon 32: F1P_EINVAL.  rho > 0, lin >= 0 and a finite margin are required, otherwise
 *   F1P_EINVAL and nothing changes. */
typedef struct f1p_kmpc_qp_avoid {
    int32_t on;              /* f1p_kmpc_qp_set_avoid: 0 turns the rows off   */
    int32_t pad;
    double margin;           /* added to every disc's radius [m] (0)          */
    double rho;              /* quadratic slack penalty (1e4)                 */
    double lin;              /* linear slack penalty (10)                     */
} f1p_kmpc_qp_avoid;
void f1p_kmpc_qp_avoid_default(f1p_kmpc_qp_avoid* avoid);
int f1p_kmpc_qp_avoid_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                            const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                            const f1p_kmpc_qp_avoid* avoid, double* steer, double* speed, int32_t* status, double* u, double* xk,
                            double* obj, double* duals, int32_t* iters, double* eps, double* planes, double* avoid_duals);
int f1p_kmpc_qp_avoid_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                          const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                          const f1p_kmpc_qp_avoid* avoid, double* d_steer, double* d_speed, int32_t* d_status, double* d_u, double* d_xk,
                          double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps, double* d_planes, double* d_avoid_duals);
int f1p_kmpc_qp_set_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* avoid);

/* Walls in the QP: the occupancy grid as SOFT, LINEARISED half-plane rows beside the discs'.  An avoidance term, not a
 * guarantee.  The problem of f1p_kmpc_qp_avoid_* is kept as it is -- the same u and the same linearisation path pbar_t, psibar_t (the
 * walk of the previous solution), the same 8T-2 plain rows, the same slack eps as input 2T with cost rho eps^2 + lin eps and the row
 * -eps <= 0, and AT MOST TWO avoidance rows per step t = 1..T, one per lane of the step.  New: per step two wall candidates compete with
 * the live discs for those two rows.  The bitmap is the ACTIVE one (f1p_set_grid dilated by f1p_inflate_grid), the cell rule the
 * collision tests' (cell = floor((p - origin) * (1 / res))); a cell outside the image or a non-finite coordinate counts as occupied.  res is
 * f1p_set_grid's and h = 0.5 * res.  For side sigma = +1 (left, slot 16) and sigma = -1 (right, slot 17):
 *   l = sigma (-sin psibar_t, cos psibar_t);
 *   the samples are q_k = pbar_t + ((double)k * h) l for k = 1 .. n_samples;
 *   k* is the first k whose q_k is occupied; if there is none, this side has no candidate;
 *   the contact is the last free sample, c = q_{k*-1}, with q_0 = pbar_t;
 *   the candidate's clearance is clear = (double)(k* - 1) * h -- pbar_t's own cell is not tested;
 *   the normal is n = -l;
 *   the row is  -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - wall_margin.
 * Selection per step: among the live discs (clear = dist - r, unchanged) and the two wall candidates the two smallest clear are taken,
 * ties to the lower slot -- discs before walls, left before right; lane j of the step takes the j-th.
 * planes[e][t][j] = (n_x, n_y, right-hand side, slot) with slots 0..15 a disc, 16 / 17 a wall, and -1 with zeros when absent;
 * avoid_duals keeps its layout.
 * The problem is feasible whenever the plain one is; statuses 1 and 3 keep their causes (the bitmap adds none); an ego with no candidate
 * at any step has the plain QP's optimum.
 * Limits: the rows are soft and linearised, an avoidance term and not a guarantee.  Two rows per step is a cap: with two discs nearer than
 * both walls at a step, that step has no wall row.  A march at res / 2 can step over the corner of a cell.  A pbar_t that already lies
 * inside the inflated wall is softly pinned between its two contacts, not pushed out.
 * Status 2 (not converged: the last iterate) is returned as for f1p_kmpc_qp_avoid_*; rows that bind with a positive slack make it more
 * frequent than in the plain QP, and the iterate is then usually the optimum to many digits.
 * Arguments: n_samples in 1..256 (else F1P_EINVAL), wall_margin (`margin`) finite, 2 <= horizon <= 31; the calls need a grid
 * (F1P_ESTATE without one) and no oriented footprint (f1p_set_footprint with n_discs > 0: F1P_ESTATE -- the rows are a point / disc
 * test, use f1p_inflate_grid).
 * f1p_kmpc_qp_walls_batch / _dev: f1p_kmpc_qp_avoid_batch / _dev with obs nullable and M in 0..16, and `walls` after `avoid` (NULL: the
 *   defaults; `on` is not read); the same outputs.
 * f1p_kmpc_qp_set_walls: NULL or on = 0 turns it off (the default).  While on, f1p_kmpc_qp_plan_batch and f1p_kmpc_qp_dev solve this
 *   problem: the discs are those of f1p_kmpc_set_obstacles[_dev], taken only while f1p_kmpc_qp_set_avoid is on as well (otherwise M = 0);
 *   rho and lin (and the discs' margin) are the context's f1p_kmpc_qp_set_avoid values whether or not it is on -- the defaults if it was
 *   never called.  The bitmap is read at launch: a later f1p_set_grid / f1p_inflate_grid is picked up by the next call. */
#define F1P_KMPC_QP_WALL_MAX_SAMPLES 256
typedef struct f1p_kmpc_qp_walls {
    int32_t on;              /* f1p_kmpc_qp_set_walls: 0 turns the rows off                       */
    int32_t n_samples;       /* samples per side, h = res / 2 apart, 1 .. 256 (48)                */
    double margin;           /* wall_margin: the rows keep this far from the contact [m] (0)     */
} f1p_kmpc_qp_walls;
void f1p_kmpc_qp_walls_default(f1p_kmpc_qp_walls* walls);
int f1p_kmpc_qp_walls_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                            const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                            const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* steer, double* speed, int32_t* status,
                            double* u, double* xk, double* obj, double* duals, int32_t* iters, double* eps, double* planes,
                            double* avoid_duals);
int f1p_kmpc_qp_walls_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                          const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                          const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* d_steer, double* d_speed,
                          int32_t* d_status, double* d_u, double* d_xk, double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps,
                          double* d_planes, double* d_avoid_duals);
int f1p_kmpc_qp_set_walls(f1p_ctx* ctx, const f1p_kmpc_qp_walls* walls);

/* ------------------------------------------------------------------------------------------------
 * Dynamic single-track MPC as the reference solves it: the linearised QP of control/dynamic_mpc/dynamic_mpc.py, batched, fp64
 * (csrc/k_stmpc_qp.hip).  Per ego:
 *   linearisation point (linear_mpc_control :995-1040): rows delta, v, yaw, yawrate, beta of predict_motion(x0, oa_prev, od_v_prev)
 *     (:279-300, update_state :317-404 with its clamps) -- the previous solution NOT shifted; zeros when NULL;
 *   model (get_dynamic_model_matrix :428-535) at (delta_t, v_t, yaw_t, yawrate_t, beta_t, oa_prev[t]): the dense 7x7 Jacobian;
 *   problem (mpc_prob_init :575-710):  min  sum_t u_t' R u_t + sum_{t<=T} (x_t - ref_t)' Q (x_t - ref_t) (Qf at T)
 *     + sum_{t<T-1} (u_{t+1} - u_t)' Rd (u_{t+1} - u_t)  s.t.  x_{t+1} = A_t x_t + B_t u_t + C_t, x_0 = x0,
 *     |u0_{t+1} - u0_t| <= MAX_STEER_V (:685, no DT factor), |delta_t| <= MAX_STEER and MIN_SPEED <= v_t <= MAX_SPEED (t = 0..T),
 *     |u0_t| <= MAX_STEER_V, |u1_t| <= MAX_ACCEL;  u = (steering speed, accel); diagonal weights only (cfg q, qf, r, rd), r > 0;
 *   output map (:1112-1117): steer = delta0 + u0_0 DT, speed = v0 + u1_0 DT.
 * Feasible iff |delta0| <= MAX_STEER and MIN_SPEED <= v0 <= MAX_SPEED (then u = 0 is feasible).  Solver, stopping rule and opts are
 * those of f1p_kmpc_qp_* (the reference's OSQP runs at eps 1e-1, :878-885; this solves its problem exactly).
 * 2 <= horizon <= F1P_STMPC_QP_MAX_T (else F1P_EINVAL).  cfg->n_rollouts is not used.
 *   x0 [E][7]; ref [E][7][T+1] (f1p_stmpc_ref_batch); oa_prev, od_v_prev [E][T] (nullable: zeros)
 * Outputs: steer, speed [E]; status [E]: 0 solved, 1 infeasible, 2 not converged (the last iterate), 3 non-finite input or model data
 *   (a predicted speed of 0 divides by v in update_state and the Jacobian); statuses 1 and 3 give NaN in every output.
 *   Nullable: u [E][T][2] (steering speed, accel), x [E][7][T+1] (the states of the linear model), obj [E] (the value cvxpy reports,
 *   the constant t = 0 term included), iters [E], and duals [E][10T-2]: the multipliers of
 *   u0_{t+1} - u0_t <= MAX_STEER_V (T-1), its negation (T-1), delta_t <= MAX_STEER for t = 1..T (T), -delta_t <= MAX_STEER (T),
 *   v_t <= MAX_SPEED (T), -v_t <= -MIN_SPEED (T), u0_t <= MAX_STEER_V (T), -u0_t (T), u1_t <= MAX_ACCEL (T), -u1_t (T)
 *   -- the reference's row order (:685-706) without the constant t = 0 rows.
 * ---------------------------------------------------------------------------------------------- */
#define F1P_STMPC_QP_MAX_T 44
int f1p_stmpc_qp_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                       const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status, double* u,
                       double* x, double* obj, double* duals, int32_t* iters);
/* the same on device buffers; asynchronous on the ctx stream */
int f1p_stmpc_qp_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev, int32_t E,
                     const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* d_steer, double* d_speed, int32_t* d_status,
                     double* d_u, double* d_x, double* d_obj, double* d_duals, int32_t* d_iters);
/* What STMPCPlanner.plan does per call with the QP solver (:133-191) for E egos in one call.  Each ego takes the kinematic branch when
 * v0 <= v_ks (:168), the dynamic one otherwise:
 *   dynamic (MPC_Control :1067-1117): reference (calc_ref_trajectory :195-233, dl) from the ctx waypoints, f1p_stmpc_qp_* on dcfg;
 *   kinematic (MPC_Control_kinematic :1176-1207): reference (calc_ref_trajectory_kinematic :237-276 with kcfg's horizon and dt, dlk;
 *     rows x, y, v, yaw), the kinematic QP of f1p_kmpc_qp_* on kcfg (STMPC's TK, DTK, Rk, Rdk, Qk, Qfk; its problem :712-833 is the
 *     kinematic planner's); output steer = delta_0 of the solution, speed = v0 + a_0 DTK.
 * The warm start is the reference's self.oa / self.odelta_v, one pair per ego shared by both branches and never shifted, kept on the
 * device with its length (0 = None): the dynamic branch restarts from zeros when the length is < T (:1005), the kinematic one when it
 * is > TK (:1052); statuses 1 and 3 reset it (the reference's None).  Requires kcfg->horizon <= dcfg->horizon (with TK > T the
 * reference's kinematic branch would linearise about a prediction cut short at the dynamic solution's length; not supported: F1P_EINVAL).
 *   x0 [E][7] host.  Outputs: steer, speed, status [E]; nullable: branch [E] (1 dynamic, 0 kinematic), obj [E], and
 *   u [E][W][2], W = max(T, TK): the new (self.oa, self.odelta_v) -- the branch's horizon of steps, NaN beyond it and for statuses 1, 3. */
int f1p_stmpc_qp_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_stmpc_cfg* dcfg, const f1p_kmpc_cfg* kcfg, double v_ks,
                            double dl, double dlk, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status,
                            int32_t* branch, double* u, double* obj);
/* the plan's warm start: forget it / read it back / install one (warm [E][W][2] fp64 = (oa, odelta_v), len [E] = its length, 0 = None) */
int f1p_stmpc_qp_warm_reset(f1p_ctx* ctx);
int f1p_stmpc_qp_warm_get(f1p_ctx* ctx, double* warm, int32_t* len, int32_t E, int32_t W);
int f1p_stmpc_qp_warm_set(f1p_ctx* ctx, const double* warm, const int32_t* len, int32_t E, int32_t W);
/* f1p_stmpc_qp_plan_batch with each ego's reference taken from its own track (track_id [E] host; needs a heading column, no raceline).
 * Ego e on track k gets outputs bit-identical to f1p_stmpc_qp_plan_batch on a ctx whose raceline is track k and which holds the same
 * warm start for e.  The warm start is the ctx's one per-ego buffer of the raceline plan (f1p_stmpc_qp_warm_*): it follows the ego,
 * not the track, as the reference's self.oa / self.odelta_v survive a change of waypoints, and the two calls may be interleaved.
 * A bad id: the ego joins neither branch, steer / speed / obj NaN, u NaN over all W steps, status F1P_ST_BAD_TRACK, branch -1, and
 * its warm start and length are neither read nor written. */
int f1p_stmpc_qp_plan_tracks_batch(f1p_ctx* ctx, const double* x0, const int32_t* track_id, int32_t E, const f1p_stmpc_cfg* dcfg,
                                   const f1p_kmpc_cfg* kcfg, double v_ks, double dl, double dlk, const f1p_kmpc_qp_opts* opts,
                                   double* steer, double* speed, int32_t* status, int32_t* branch, double* u, double* obj);

/* Moving-disc avoidance in the dynamic QP: f1p_stmpc_set_obstacles' discs as SOFT, LINEARISED half-plane rows, the
 * dynamic twin of f1p_kmpc_qp_avoid_* with the same struct and defaults (f1p_kmpc_qp_avoid, f1p_kmpc_qp_avoid_default).  An avoidance
 * term, not a guarantee.  The problem of f1p_stmpc_qp_* is kept -- u = (steer_v_0, accel_0, ...), the linearisation about
 * predict_motion(x0, oa_prev, od_v_prev), the same 10T-2 rows -- and gains
 *   one slack eps: cost rho eps^2 + lin eps, uncoupled from u in H, row -eps <= 0;
 *   at most two rows per step t = 1..T.  pbar_t: the position of the linearisation path after t steps (update_state with its clamps,
 *     t = T included).  A live slot (r >= 0) is predicted at tau = (double)t * DT: c = (x + vx tau, y + vy tau), d = pbar_t - c,
 *     dist = sqrt(dx^2 + dy^2), clear = dist - r.  The two live slots with the smallest clear are taken, ties to the lower slot; each
 *     gives the normal n = d / dist (dist < 1e-9: n = -(cos, sin)(psibar_t + betabar_t), the direction of travel: stay behind it) and,
 *     with x_t = S(t) u + s(t) the linear model's state (rows 0 and 1: x and y), the row
 *       -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - (r + margin).
 * An empty slot is r < 0 or r NaN; an ego without a live slot has no such row and the optimum of f1p_stmpc_qp_* (eps = 0).  A live slot
 * with a non-finite number: status 3.  Status 1 as for f1p_stmpc_qp_* (|delta0| > MAX_STEER or v0 outside its bounds).
 * 2 <= horizon <= F1P_STMPC_QP_AVOID_MAX_T (the longest horizon whose LDS layout, the packed avoidance rows included, one workgroup may
 * claim; else F1P_EINVAL).  The warm start stays (oa, odelta_v); eps is not carried.  obj includes rho eps^2 + lin eps.
 * f1p_stmpc_qp_avoid_batch / _dev: f1p_stmpc_qp_batch / _dev with obs [E][M][5] (M in 1..16) and avoid (NULL: the defaults; `on` is not
 *   read), and the nullable outputs eps [E]; planes [E][T][2][4] = (n_x, n_y, right-hand side, slot as a double; slot -1 and zeros for an
 *   absent row); avoid_duals [E][2T+1]: the multipliers of the 2T avoidance rows in step order (0 for an absent row), then of -eps <= 0.
 *   duals [E][10T-2] keeps its layout.  Statuses 1 and 3: NaN in all of them.
 * f1p_stmpc_qp_set_avoid: a switch of its own beside f1p_kmpc_qp_set_avoid; NULL or on = 0 turns it off (the default).  While on,
 *   f1p_stmpc_qp_dev, f1p_stmpc_qp_plan_batch and f1p_stmpc_qp_plan_tracks_batch solve this problem with the discs held by
 *   f1p_stmpc_set_obstacles[_dev] (none held: no avoidance rows), which are in the CALLER'S ego order: each branch of a plan gets its
 *   egos' rows gathered on the device.  The plan's kinematic branch solves f1p_kmpc_qp_avoid_*'s problem on kcfg with the same discs and
 *   numbers, whatever f1p_kmpc_qp_set_avoid says: kcfg->horizon <= 31.  A plan whose E is not the E the obstacles were set for:
 *   F1P_ESTATE; a horizon past either cap: F1P_EINVAL.  rho > 0, lin >= 0 and a finite margin are required, otherwise F1P_EINVAL and
 *   nothing changes.  Off: every entry point is what it is without this call. */
#define F1P_STMPC_QP_AVOID_MAX_T 40
int f1p_stmpc_qp_avoid_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                             const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                             const f1p_kmpc_qp_avoid* avoid, double* steer, double* speed, int32_t* status, double* u, double* x,
                             double* obj, double* duals, int32_t* iters, double* eps, double* planes, double* avoid_duals);
int f1p_stmpc_qp_avoid_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev,
                           int32_t E, const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                           const f1p_kmpc_qp_avoid* avoid, double* d_steer, double* d_speed, int32_t* d_status, double* d_u, double* d_x,
                           double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps, double* d_planes, double* d_avoid_duals);
int f1p_stmpc_qp_set_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* avoid);
/* bytes of LDS one ego's workgroup of the avoidance variant claims at this horizon (F1P_STMPC_QP_AVOID_MAX_T is the longest that fits the
 * CU; above 64 KiB the kernel is opted in to the larger allocation, a launch path of its own); -1: horizon < 2.  Needs no context. */
int64_t f1p_stmpc_qp_avoid_lds_bytes(int32_t horizon);

/* Walls in the dynamic QP: the occupancy grid as SOFT, LINEARISED half-plane rows beside the discs', the dynamic twin of
 * f1p_kmpc_qp_walls_* with the same struct and defaults (f1p_kmpc_qp_walls, f1p_kmpc_qp_walls_default).  An avoidance term, not a
 * guarantee.  The problem of f1p_stmpc_qp_avoid_* is kept as it is -- the same u, the linearisation about predict_motion(x0, oa_prev,
 * od_v_prev), the same 10T-2 plain rows, the same slack eps (cost rho eps^2 + lin eps, row -eps <= 0, solved for scaled by
 * 1 / sqrt(2 rho)) and AT MOST TWO avoidance rows per step t = 1..T.  New: per step two wall candidates compete with the live discs for
 * those two rows.  The bitmap is the ACTIVE one (f1p_set_grid dilated by f1p_inflate_grid), the cell rule the collision tests'
 * (cell = floor((p - origin) * (1 / res))); a cell outside the image or a non-finite coordinate counts as occupied.  res is f1p_set_grid's
 * and h = 0.5 * res.  pbar_t is the linearisation path's position after t steps and w_t = psibar_t + betabar_t its direction of travel
 * there (yaw + slip angle: the angle f1p_stmpc_qp_avoid_*'s on-centre normal uses, NOT the bare yaw).  For side sigma = +1 (left, slot
 * 16) and sigma = -1 (right, slot 17):
 *   l = sigma (-sin w_t, cos w_t);
 *   the samples are q_k = pbar_t + ((double)k * h) l for k = 1 .. n_samples;
 *   k* is the first k whose q_k is occupied; if there is none, this side has no candidate;
 *   the contact is the last free sample, c = q_{k*-1}, with q_0 = pbar_t;
 *   the candidate's clearance is clear = (double)(k* - 1) * h -- pbar_t's own cell is not tested;
 *   the normal is n = -l;
 *   the row is  -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - wall_margin.
 * Selection per step: of {the live disc with the least clear = dist - r, the one with the second least, wall L, wall R} the two smallest
 * clear are taken, ties to the lower slot -- discs before walls, left before right; the step's first row is the first of them.
 * planes[e][t][j] = (n_x, n_y, right-hand side, slot) with slots 0..15 a disc, 16 / 17 a wall, and -1 with zeros when absent;
 * avoid_duals keeps its layout.
 * The problem is feasible whenever the plain one is; statuses 1 and 3 keep their causes (the bitmap adds none); an ego with no candidate
 * at any step has the optimum of f1p_stmpc_qp_avoid_* (of f1p_stmpc_qp_* without a live disc).  The limits are f1p_kmpc_qp_walls_*'s:
 * soft and linearised rows, two rows per step, a march that can step over a cell's corner, a pbar_t inside the wall pinned and not pushed
 * out; status 2 as there.
 * Arguments: n_samples in 1..256 (else F1P_EINVAL), wall_margin (`margin`) finite, 2 <= horizon <= F1P_STMPC_QP_AVOID_MAX_T; the calls
 * need a grid (F1P_ESTATE without one) and no oriented footprint (f1p_set_footprint with n_discs > 0: F1P_ESTATE).
 * f1p_stmpc_qp_walls_batch / _dev: f1p_stmpc_qp_avoid_batch / _dev with obs nullable and M in 0..16, and `walls` after `avoid` (NULL: the
 *   defaults; `on` is not read); the same outputs.
 * f1p_stmpc_qp_set_walls: a switch of its own beside f1p_kmpc_qp_set_walls; NULL or on = 0 turns it off (the default).  While on,
 *   f1p_stmpc_qp_dev, f1p_stmpc_qp_plan_batch and f1p_stmpc_qp_plan_tracks_batch solve this problem in both branches: the dynamic egos
 *   here, the kinematic ones f1p_kmpc_qp_walls_*'s problem on kcfg with the same numbers (kcfg->horizon <= 31, horizon <=
 *   F1P_STMPC_QP_AVOID_MAX_T, else F1P_EINVAL).  The discs are those of f1p_stmpc_set_obstacles[_dev], taken only while
 *   f1p_stmpc_qp_set_avoid is on as well (otherwise M = 0); rho and lin (and the discs' margin) are the context's f1p_stmpc_qp_set_avoid
 *   values whether or not it is on -- the defaults if it was never called.  The bitmap is read at launch: a later f1p_set_grid /
 *   f1p_inflate_grid is picked up by the next call.  Off: every entry point is what it is without this call. */
int f1p_stmpc_qp_walls_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                             const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                             const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* steer, double* speed, int32_t* status,
                             double* u, double* x, double* obj, double* duals, int32_t* iters, double* eps, double* planes,
                             double* avoid_duals);
int f1p_stmpc_qp_walls_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev,
                           int32_t E, const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                           const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* d_steer, double* d_speed,
                           int32_t* d_status, double* d_u, double* d_x, double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps,
                           double* d_planes, double* d_avoid_duals);
int f1p_stmpc_qp_set_walls(f1p_ctx* ctx, const f1p_kmpc_qp_walls* walls);

/* ------------------------------------------------------------------------------------------------
 * SURVEY.md 8f rank 2 -- the dynamic single-track model as a second model for shooting MPC
 * (control/dynamic_mpc/dynamic_mpc.py): predict_motion / update_state (:280-404), calc_ref_trajectory (:195-233),
 * objective :616-622, bounds :685-706, output map :1112-1117.
 *   x0 [E][7]; oa / od_v [E][T] fp64; path [E][7][T+1]; states [E][4] = (x, y, v, yaw); ref [E][7][T+1];
 *   controls [E][T][2][R] f32 = (steering speed, accel), rollout index fastest.  +-inf is clamped to the bound; a NaN stays a NaN (the rule of
 *   f1p_kmpc_shoot_*'s controls: the first rollout with a NaN control wins with a NaN cost, in both evaluation modes).
 * ---------------------------------------------------------------------------------------------- */
int f1p_stmpc_predict_batch(f1p_ctx* ctx, const double* x0, const double* oa, const double* od_v, int32_t E,
                            const f1p_stmpc_cfg* cfg, double* path);
int f1p_stmpc_ref_batch(f1p_ctx* ctx, const double* states, int32_t E, int32_t horizon, double dt, double dl, double* ref);
/* Evaluation mode of f1p_stmpc_shoot_*: mixed = 1 (default) an f32 filter over every rollout + fp64 re-evaluation of the rollouts
 * that can still be the minimum (those within the margin of the f32 minimum, and every rollout whose speed leaves the range in
 * which the reference's explicit-Euler step is stable with margin: v < 1.88 m/s for the default vehicle), decision on the fp64 costs -- outputs
 * bit-identical to mixed = 0 (plain fp64).  d_cost32 [E][R] f32 (-inf = untrusted) and d_n_refined [E] i32 (-1 = the ego fell back
 * to all fp64): device pointers, nullable test hooks. */
int f1p_stmpc_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_n_refined);
/* Occupancy test on the rollouts of the dynamic MPC's shooting solver; f1p_kmpc_set_collision's twin, with a state of
 * its own: one context may run both planners with different settings.
 * on = 0 (default): rollouts are not tested, and the launch path selects the kernels it selects without this call.  on = 1: a rollout of
 * f1p_stmpc_plan_* / f1p_stmpc_shoot_* whose tested points touch an occupied cell cannot win.  n_sub in [1, 16]: points tested per step
 * of the dynamic model (a step covers at most max_speed * dt = 0.15 m); n_sub_k in [1, 16]: per step of f1p_stmpc_plan_batch's
 * kinematic branch (TK steps of DTK = 0.1 s).
 * Tested points (dynamic branch): with p_0 .. p_T the (x, y) of the states the fp64 rollout visits under the APPLIED controls (dv and a
 * clamped to their bounds, dv to pdv +- max_steer_v for t > 0), for t = 0 .. T-1 and j = 1 .. n_sub the point
 * p_t + (p_{t+1} - p_t) * ((double)j / (double)n_sub), per coordinate in fp64 in that order; j = n_sub is p_{t+1} itself; p_0 is not
 * tested.  The kinematic branch: f1p_kmpc_set_collision's rule with n_sub_k.
 * Cell rule: f1p_kmpc_set_collision's -- the ACTIVE bitmap (f1p_inflate_grid(r) makes it a disc test); outside the image or a
 * non-finite coordinate is occupied.
 * Decision: first minimum by rollout index over the unblocked rollouts (NaN costs as without the test).  Every rollout blocked:
 * best_idx = -1, best_cost = +inf, steer = 0, speed = 0, best_seq all zero, the ego's warm-start row zero; its warm-start tag stays
 * the branch's own.  A blocked ego has no effect on any other ego.
 * f1p_stmpc_plan_* in the mixed mode runs an f32 filter that only decides what cannot win (its tested points looked up in the clearance
 * map; used while the derived f32 position bound, with 5x headroom, stays below one cell -- otherwise plain fp64); outputs are
 * bit-identical to f1p_stmpc_set_mode(0).  f1p_stmpc_shoot_* (streamed controls) with the test on are evaluated in plain fp64 WHATEVER
 * f1p_stmpc_set_mode says; with the same controls they equal f1p_stmpc_plan_dev bit for bit (f1p_stmpc_gen_controls_dev).  The
 * kinematic branch runs f1p_kmpc_plan_*'s schedule with the test (k_kmpc_plan_gen_idx_col) under f1p_kmpc_set_mode.
 * With the test on, f1p_stmpc_plan_dev, f1p_stmpc_plan_batch, f1p_stmpc_shoot_dev and f1p_stmpc_shoot_batch return an error, launch
 * nothing and leave the warm-start tags alone when no grid is loaded (F1P_ESTATE), when an oriented footprint is installed
 * (f1p_set_footprint with n_discs > 0; F1P_ESTATE) or, f1p_stmpc_plan_batch only, when f1p_kmpc_set_groups(> 0) is in force
 * (F1P_ESTATE).  A count outside [1, 16]: F1P_EINVAL, the switch keeps its state.
 * Not covered: f1p_stmpc_qp_* (the QP has no rollouts to test; the grid is not among its constraints). */
int f1p_stmpc_set_collision(f1p_ctx* ctx, int32_t on, int32_t n_sub, int32_t n_sub_k);
/* Moving obstacles on the rollouts of the dynamic MPC's shooting solver: f1p_kmpc_set_obstacles' discs and rule
 * for f1p_stmpc_*.  obs [E][M][5] fp64 rows (x, y, vx, vy, r) in the map frame, M <= F1P_KMPC_MAX_OBS, INDEXED BY THE CALLER'S EGO
 * ORDER (for f1p_stmpc_plan_batch the batch's, whatever branch an ego takes); a slot with !(r >= 0) is empty.
 * Tested points: f1p_stmpc_set_collision's, n_sub per step of the dynamic model and n_sub_k per step of plan_batch's kinematic
 * branch (the context keeps both numbers while `on` is 0; defaults 1 and 2).  The point of step t at f = (double)j / (double)n_sub
 * has the time tau = ((double)t + f) * dt with the BRANCH's dt; against a live slot, in fp64 and in this order,
 *   cx = x + vx * tau; cy = y + vy * tau; dx = Px - cx; dy = Py - cy; d2 = dx*dx + dy*dy;   blocked when !(d2 > r*r)
 * -- touching blocks, a NaN anywhere blocks.  With f1p_stmpc_set_collision on as well a point is tested against both rules.  The
 * decision, the NaN-cost rule and the all-blocked outputs (best_idx -1, best_cost +inf, steer 0, speed 0, zero best_seq, zero warm
 * row, the warm tag the branch's own) are that test's.  An ego without a live slot gets the bits of the plan without obstacles.
 * f1p_stmpc_set_obstacles copies the array on the context's stream; obs == NULL or M == 0 clears.  f1p_stmpc_set_obstacles_dev
 * BORROWS a device array: the caller keeps it alive and may rewrite it in place between plans (in stream order).  The obstacles
 * are a state of their own beside f1p_kmpc_set_obstacles' (f1p_kmpc_* follows that one only, f1p_stmpc_* this one only) and
 * apply to f1p_stmpc_plan_dev / _plan_batch / _shoot_dev / _shoot_batch with or without a grid; the streamed entry points are then
 * evaluated in plain fp64 whatever the mode and equal f1p_stmpc_plan_dev bit for bit.
 * Errors, nothing launched and no warm tag touched: M outside [1, 16]: F1P_EINVAL; a plan whose E is not the obstacles' E (for
 * plan_batch the caller's E): F1P_ESTATE; f1p_stmpc_plan_batch under f1p_kmpc_set_groups(> 0) with obstacles set: F1P_ESTATE.
 * f1p_stmpc_qp_dev / f1p_stmpc_qp_plan_batch / f1p_stmpc_qp_plan_tracks_batch take the same discs as soft half-plane rows of the QP
 * while f1p_stmpc_qp_set_avoid is on (above), and ignore them while it is off.
 * Not covered: a MultiContext's sharded plans, f1p_kmpc_*. */
int f1p_stmpc_set_obstacles(f1p_ctx* ctx, const double* obs, int32_t E, int32_t M);
int f1p_stmpc_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, int32_t E, int32_t M);
int f1p_stmpc_shoot_batch(f1p_ctx* ctx, const double* x0, const double* ref, const float* controls, int32_t E,
                          const f1p_stmpc_cfg* cfg, double* steer, double* speed, int32_t* best_idx, double* best_cost,
                          double* best_seq);
int f1p_stmpc_shoot_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, int32_t E,
                        const f1p_stmpc_cfg* cfg, double* d_steer, double* d_speed, int32_t* d_best_idx,
                        double* d_best_cost, double* d_best_seq);

/* ------------------------------------------------------------------------------------------------
 * The dynamic MPC's shooting solver with the controls GENERATED IN THE KERNEL and a per-ego warm start kept on the device
 * (STMPCPlanner.plan with SOLVER = "shooting", batched; csrc/k_stmpc.hip).  The generator is f1p_kmpc_plan_*'s:
 * control (rollout r, step t) of ego e = Philox4x32-10(counter (t / 2, r, e, call), key seed) -> standardised Irwin-Hall byte
 * sums z -> fma(sigma_c, z_c, warm_c[t]) per channel c; rollout 0 = the warm start itself, rollout 1 = all zero (CPU restatement:
 * oracle/f1p_oracle.c orc_kmpc_gen_controls).  Dynamic model (v > V_KS, MPC_Control :1067-1117): channel 0 = steering speed
 * (sigma_steer_v), channel 1 = accel (sigma_accel); kinematic model (v <= V_KS, MPC_Control_kinematic :1012-1063): channel 0 = accel
 * (sigma_accel), channel 1 = steering angle (sigma_steer).  The ego word e is the ego's index in the caller's batch + ego_offset
 * (a batch that is one shard of a larger one passes its first ego's global index), in both branches: an ego's plan is a function of
 * that ego alone, wherever it stands in the batch and whatever the others do.
 * A struct of its own rather than f1p_kmpc_sampler used twice: the two branches share seed, call and use_warm, which two samplers
 * could set apart by mistake, and the ego offset has no place in the kinematic one.
 *   f1p_stmpc_gen_controls_dev + f1p_stmpc_shoot_dev  ==  f1p_stmpc_plan_dev   bit for bit (tests/test_gpu_stmpc_plan.py),
 *   under both settings of f1p_stmpc_set_mode.
 * Warm start: f32 [E][W][2], W = max(T, TK), plus a tag per ego -- 0: none, 1: written by the kinematic branch ([TK][2] = (accel,
 * steer)), 2: by the dynamic branch ([T][2] = (steering speed, accel)); rows past the branch's horizon are unspecified.  After a plan
 * the row is the winner's APPLIED sequence (after the bound projection :685-706 / :391-401) shifted by one step, last step repeated,
 * rounded to f32 (what :1052-1055 / :1005-1008 keep in self.oa / self.odelta_v).  An ego whose tag is not its branch's starts from
 * zeros (the channels mean different things), as does every ego with use_warm = 0, after f1p_stmpc_warm_reset and after a change of
 * E, T or TK.  Separate from f1p_kmpc_warm_* and from the QP's f1p_stmpc_qp_warm_*.
 * ---------------------------------------------------------------------------------------------- */
typedef struct f1p_stmpc_sampler {
    uint64_t seed;         /* Philox key */
    uint32_t call;         /* plan counter: advance per plan */
    int32_t use_warm;      /* 0: generate around zeros (the warm start is still written) */
    double sigma_steer_v;  /* dynamic branch, channel 0 [rad/s] */
    double sigma_accel;    /* both branches [m/s^2] */
    double sigma_steer;    /* kinematic branch, channel 1 [rad] */
    int32_t ego_offset;    /* added to the batch index in the generator's ego word (>= 0) */
    int32_t reserved;      /* 0 */
} f1p_stmpc_sampler;
/* the controls the next f1p_stmpc_plan_dev of this shape would evaluate, as the [E][T][2][R] f32 buffer f1p_stmpc_shoot_dev takes
 * (dynamic_mpc.py:685-706 are applied by the rollouts, not here); asynchronous.  Does not change the warm start. */
int f1p_stmpc_gen_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_stmpc_cfg* cfg, const f1p_stmpc_sampler* smp);
/* MPC_Control (:1067-1117) by shooting on a given reference, dynamic model for every ego: d_x0 [E][7], d_ref [E][7][T+1]
 * (f1p_stmpc_ref_*_dev); outputs as f1p_stmpc_shoot_dev (d_best_cost, d_best_seq nullable).  Asynchronous on the ctx stream; the
 * f32 filter / fp64 refinement / decision schedule of f1p_stmpc_shoot_dev with no controls buffer anywhere. */
int f1p_stmpc_plan_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, int32_t E, const f1p_stmpc_cfg* cfg,
                       const f1p_stmpc_sampler* smp, double* d_steer, double* d_speed, int32_t* d_best_idx, double* d_best_cost,
                       double* d_best_seq);
/* STMPCPlanner.plan (:152-191) by shooting for a batch, host arrays: x0 [E][7]; per ego the model switch of :168 (v <= v_ks:
 * kinematic model on kcfg, reference rows 0, 1, 3, 4 of calc_ref_trajectory :195-233 with (TK, DTK, dlk); else the dynamic model
 * on dcfg with (T, DT, dl)), reference extraction from the ctx waypoints, plan, warm-start update.  branch [E] (nullable): 0
 * kinematic, 1 dynamic.  best_seq [E][W][2] (nullable), W = max(T, TK): the winner's applied sequence in its branch's channel order,
 * NaN past the branch's horizon.  best_cost nullable. */
int f1p_stmpc_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_stmpc_cfg* dcfg, const f1p_kmpc_cfg* kcfg, double v_ks,
                         double dl, double dlk, const f1p_stmpc_sampler* smp, double* steer, double* speed, int32_t* best_idx,
                         double* best_cost, int32_t* branch, double* best_seq);
/* the warm start of f1p_stmpc_plan_* (:1052-1055, :1005-1008): warm [E][W][2] f32, tag [E] i32, host arrays, W = max(T, TK)
 * (TK = 0 for a ctx that only runs f1p_stmpc_plan_dev) */
int f1p_stmpc_warm_reset(f1p_ctx* ctx);
int f1p_stmpc_warm_get(f1p_ctx* ctx, float* warm, int32_t* tag, int32_t E, int32_t T, int32_t TK);
int f1p_stmpc_warm_set(f1p_ctx* ctx, const float* warm, const int32_t* tag, int32_t E, int32_t T, int32_t TK);

/* ------------------------------------------------------------------------------------------------
 * Rivals: each ego's nearest other vehicles as moving discs, on the device (csrc/k_rivals.hip).  The output is the
 * [E][M][5] array (and, for the lattice, the pace [E]) that f1p_kmpc_set_obstacles_dev, f1p_stmpc_set_obstacles_dev and
 * f1p_lattice_set_obstacles_dev borrow.
 * Inputs.
 *   - E vehicle states in one of three layouts:
 *       F1P_RIVALS_XYVYAW = 0: [E][4] = (x, y, v, yaw), the kinematic MPC's x0; heading h = yaw.
 *       F1P_RIVALS_POSE = 1: [E][4] = (x, y, theta, v), the lattice poses; h = theta.
 *       F1P_RIVALS_ST7 = 2: [E][7] = (x, y, delta, v, yaw, yaw_rate, beta), the dynamic MPC's x0; h = yaw + beta, one fp64 add.
 *   - An optional group id per ego, group[e] int32, any values (f1p_rivals_set_groups).
 *       Egos with the same id >= 0 are one race.
 *       An ego with a negative id has no rivals and is nobody's rival.
 *       No groups means one race of all E.
 *   - M in [1, 16], radius >= 0, reach >= 0 (+inf allowed), min_speed > 0.
 * Selection, for ego i with group[i] >= 0, over every j != i with group[j] == group[i].
 *   - dx = x_j - x_i; dy = y_j - y_i; d2 = dx*dx + dy*dy, in fp64, no contraction.
 *   - j is a candidate unless d2 > reach*reach.
 *       reach*reach is formed once on the host in fp64.
 *       A NaN d2 is a candidate.
 *   - Candidates are ordered by the project's np.argmin rule, applied repeatedly: NaN d2 first, then ascending d2, then ascending j
 *     on equal bits.
 *       Coincident vehicles (d2 == 0) are ordinary candidates.
 *   - The first min(M, #candidates) become slots 0, 1, ... in that order.
 *   - The remaining slots are empty.
 * Slot values.
 *   - Live slot: (x_j, y_j, v_j*cos(h_j), v_j*sin(h_j), radius).
 *       x, y and r are bit copies.
 *       The trig is the full-range device sincos, not sincos_core, because a heading is unbounded here.
 *   - Empty slot: (0, 0, 0, 0, -1.0).
 * Other outputs.
 *   - idx[e][m] int32: the chosen j, or -1.
 *   - pace[e]: m = fabs(v_e); if !(m >= min_speed) then m = (m != m) ? m : min_speed; pace = 1.0 / m.
 *       Bit-equal to 1.0 / np.maximum(np.abs(v), min_speed), which is what LatticePlanner forms on the host for explicit obstacles.
 *       A NaN speed gives a NaN pace, which blocks that ego's candidates.
 * NaN policy: NaN sorts first and therefore blocks, the library's rule everywhere ("a NaN anywhere blocks").  A vehicle with a NaN
 * position has a NaN d2 to every member of its race (its own rivals included), so it takes slot 0 of each of them and its NaN slot
 * values block every rollout / candidate there: ONE vehicle with a NaN position blocks its WHOLE race, and only its race.
 *
 * f1p_rivals_set_groups builds the member list sorted by (group, ego) and each ego's [begin, end) in it on the host and keeps them in
 * device buffers of the context (synchronous); group == NULL returns to one race of all (any E).
 * f1p_rivals_dev is asynchronous on the context's stream and owns nothing: it can write straight into the arrays the three
 * *_set_obstacles_dev borrow.  d_pace and d_idx are nullable.  f1p_rivals_batch: the same on host arrays, synchronous.
 * Errors, nothing launched: a bad layout, M outside [1, 16], !(radius >= 0), !(reach >= 0), !(min_speed > 0), E < 1 or a NULL states /
 * obs array (for set_groups: E < 1 with a group array): F1P_EINVAL; E different from the E the groups were set for: F1P_ESTATE.
 * E == 1 is valid: every slot is empty.
 * ---------------------------------------------------------------------------------------------- */
#define F1P_RIVALS_XYVYAW 0
#define F1P_RIVALS_POSE 1
#define F1P_RIVALS_ST7 2
#define F1P_RIVALS_MAX 16
int f1p_rivals_set_groups(f1p_ctx* ctx, const int32_t* group, int32_t E);
int f1p_rivals_dev(f1p_ctx* ctx, const double* d_states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                   double min_speed, double* d_obs, double* d_pace, int32_t* d_idx);
int f1p_rivals_batch(f1p_ctx* ctx, const double* states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                     double min_speed, double* obs, double* pace, int32_t* idx);

/* ------------------------------------------------------------------------------------------------
 * Rivals, predicted along the course (csrc/k_rivals_predict.hip).  A rival that follows a raceline stays on it: instead of
 * the constant-velocity (vx, vy) above, a live slot carries the CHORD of the rival's path along its course over the ego's horizon, and a
 * radius optionally widened by the largest distance between that path and the chord.  Selection, slot order, idx, pace, empty slots,
 * groups, reach and the NaN ordering are exactly those above; only vx, vy, r of a LIVE slot change.
 * Course of vehicle j: the polyline p_0 .. p_{n-1} (x and y columns) of the context's raceline, or of track track_id[j] of the context's
 * track set (f1p_rivals_set_course).  All in fp64, no contraction:
 *   - len_k = sqrt(dx*dx + dy*dy); cum_0 = 0; cum_{k+1} = cum_k + len_k, added one by one in index order; L = cum_{n-1}.
 *   - u_k = (p_{k+1} - p_k) / len_k (each component divided); left normal n_k = (-u_k.y, u_k.x).
 * Frenet record of vehicle j, once per vehicle per call:
 *   - (b, t, q): segment index, parameter and projection that f1p_nearest_point_batch / f1p_nearest_point_tracks_batch return for
 *     (x_j, y_j) on that course -- the same device functions, the same bits.
 *   - s0 = cum_b + t * len_b;  d = (x_j - q.x) * n_b.x + (y_j - q.y) * n_b.y.
 *   - dir = (v_j * (cos h_j * u_b.x + sin h_j * u_b.y) >= 0) ? +1 : -1, h_j the layout's heading as above (full-range sincos).
 * Position at time tau:
 *   - s = s0 + (dir * |v_j|) * tau;  with wrap: s = s - L * floor(s / L);  in both modes s is then clamped into [0, L].
 *   - k = the largest index <= n - 2 with cum_k <= s (a binary search).
 *   - P(tau) = p_k + u_k * (s - cum_k) + n_k * d, per component, left to right.
 *     wrap jumps from p_{n-1} to p_0 without a closing segment (the reference's single index wrap, kinematic_mpc.py:194).
 * Slot of ego i that holds vehicle j:
 *   - H_i = horizon_s + horizon_m * pace_i, pace_i as above;  knots c_k = P((H_i * k) / K), k = 0 .. K, K = knots.
 *   - x, y: bit copies of x_j, y_j, as above.
 *   - vx = (c_K.x - c_0.x) / H_i, vy likewise.
 *   - dev = max over 0 < k < K of sqrt(ex*ex + ey*ey), e = (c_k - c_0) - (c_K - c_0) * (k / K);  0 for K = 1.
 *   - r = radius + dev with inflate, else radius (a bit copy).
 * The slot keeps the constant-velocity bits above when x_j, y_j, v_j, h_j or H_i is not finite, !(H_i > 0), !(|v_j| * H_i < 1e9),
 * track_id[j] is outside [0, K_tracks), or the course has a zero-length segment or an L that is not finite and positive -- so the NaN
 * policy ("a NaN anywhere blocks") is exactly the one above.
 *
 * f1p_rivals_set_course: track_id host [E], vehicle j follows track track_id[j] of the track set in force at the following calls
 * (synchronous, kept in a device buffer of the context); NULL (any E): every vehicle follows the context's raceline, the default.
 * f1p_rivals_predict_dev: asynchronous on the context's stream; d_pace, d_idx and d_frenet are nullable.  d_frenet [E][3] =
 * (s0, d, dir) per vehicle, a NaN row for a vehicle that falls back for a cause of its own (state, track id, course).  The arc tables
 * live in buffers of the context and are rebuilt, by one launch, when f1p_set_waypoints* / f1p_set_track_set has been called since.
 * f1p_rivals_predict_batch: the same on host arrays, synchronous.
 * Errors, nothing launched: everything f1p_rivals_dev rejects, knots outside [1, 16], a negative or NaN horizon_s / horizon_m, both
 * zero, a speed other than the two below, a NULL pr (set_course: E < 1 with an id array): F1P_EINVAL; E different from the E the
 * courses were set for, or no track set (ids set) / no raceline (no ids): F1P_ESTATE.
 *
 * Rivals, predicted with the course's speed profile (speed = F1P_RIVALS_SPEED_PROFILE).  With speed =
 * F1P_RIVALS_SPEED_CONSTANT (0, the default) a rival keeps |v_j| along its course, the rule above.  With F1P_RIVALS_SPEED_PROFILE it
 * advances in the course's TIME coordinate, scaled by how fast it is going now relative to the course's speed where it stands: a rival at
 * raceline speed brakes and accelerates with the raceline, one at 80 % does 80 % of it, a standing one stands.  Everything above stays;
 * only the map from tau to a point on the course changes.  All in fp64, in this operation order, no contraction.
 * Per course, w_k its speed column (the raceline's / the track's v column), len_k and cum_k as above, floor = the call's min_speed:
 *   - c_k = 0.5 * (|w_k| + |w_{k+1}|), k = 0 .. n-2;  if !(c_k >= floor) then c_k = floor.
 *   - tim_0 = 0; tim_{k+1} = tim_k + len_k / c_k, added one by one in index order; Tl = tim_{n-1}.
 *   - The course is PROFILE-USABLE if it is usable in the sense above, every w_k is finite and Tl is finite and positive.
 * Per vehicle j with Frenet record (s0, d, dir, b):
 *   - rho = |v_j| / c_b;  th0 = tim_b + (s0 - cum_b) / c_b.
 * Position at time tau:
 *   - th = th0 + (dir * rho) * tau;  with wrap: th = th - Tl * floor(th / Tl);  in both modes th is then clamped into [0, Tl].
 *   - k = the largest index <= n - 2 with tim_k <= th (a binary search in tim).
 *   - P(tau) = p_k + u_k * ((th - tim_k) * c_k) + n_k * d, per component, left to right.
 * A vehicle on a course that is usable but not profile-usable is predicted by the constant-speed rule: its slots are bit-equal to the
 * same call with speed = F1P_RIVALS_SPEED_CONSTANT.  Every other fallback is unchanged and keeps the constant-velocity bits.
 * The time tables live next to the arc tables, are built only when a profile call asks for them, and are rebuilt, by one launch, when
 * the course has been replaced since or the call's min_speed differs from the one they were built with.
 * ---------------------------------------------------------------------------------------------- */
#define F1P_RIVALS_KNOTS_MAX 16
#define F1P_RIVALS_SPEED_CONSTANT 0
#define F1P_RIVALS_SPEED_PROFILE 1
typedef struct f1p_rivals_predict {
    double horizon_s;              /* H_i = horizon_s [s] + horizon_m [m] * pace_i */
    double horizon_m;
    int32_t knots;                 /* K in [1, 16] */
    int32_t inflate;               /* != 0: r = radius + dev */
    int32_t wrap;                  /* != 0: the course is a loop */
    int32_t speed;                 /* F1P_RIVALS_SPEED_CONSTANT (0): |v_j| along the course; F1P_RIVALS_SPEED_PROFILE: the course's speed profile */
} f1p_rivals_predict;
int f1p_rivals_set_course(f1p_ctx* ctx, const int32_t* track_id, int32_t E);
int f1p_rivals_predict_dev(f1p_ctx* ctx, const double* d_states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                           double min_speed, const f1p_rivals_predict* pr, double* d_obs, double* d_pace, int32_t* d_idx,
                           double* d_frenet);
int f1p_rivals_predict_batch(f1p_ctx* ctx, const double* states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                             double min_speed, const f1p_rivals_predict* pr, double* obs, double* pace, int32_t* idx, double* frenet);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: egos shard with no communication (one ctx per rank).  Only when ONE ego's candidate set is
 * split over ranks is there an exchange step: all-reduce(min) of the per-ego best cost, then
 * all-reduce(min) of the candidate index among the ranks that hold that cost (np.argmin first-minimum
 * rule, lattice_planner.py:159-172), both RCCL collectives enqueued on the ctx stream.
 * ---------------------------------------------------------------------------------------------- */
#define F1P_COMM_ID_BYTES 128
int f1p_comm_unique_id(f1p_ctx* ctx, uint8_t id[F1P_COMM_ID_BYTES]);              /* rank 0, then broadcast */
int f1p_comm_init(f1p_ctx* ctx, const uint8_t id[F1P_COMM_ID_BYTES], int32_t nranks, int32_t rank);
int f1p_comm_destroy(f1p_ctx* ctx);
/* number of ranks / this rank as the RCCL communicator itself reports them (ncclCommCount / ncclCommUserRank) */
int f1p_comm_info(f1p_ctx* ctx, int32_t* nranks, int32_t* rank);
/* in place on device buffers: d_cost [E] fp64 <- global min; d_idx [E] int32 <- lowest index with that cost.
 * np.argmin's ordering including its NaN rule (a NaN cost wins, the first one by index): the cost is reduced as a
 * monotone unsigned 64-bit key (NaN -> 0), so both collectives are integer all-reduce(min) and every rank agrees. */
int f1p_comm_argmin_dev(f1p_ctx* ctx, double* d_cost, int32_t* d_idx, int32_t E);
/* Form of the exchange inside f1p_comm_argmin_dev.  0 (default): two dependent RCCL all-reduces -- min over the u64 cost keys, then min over
 * the i32 indices of the ranks holding that key (12 B per ego on the wire, two collective latencies).  1: ONE all-gather of (key, index)
 * records (16 B per ego and rank) and a local minimum by the same (key, index) order on every rank -- the same result bit for bit, one
 * collective latency; the better trade once the exchange is latency-bound (4096 egos x 8 ranks = 512 KB gathered per rank).
 * f1p_argmin_gather_reduce_batch runs the local kernels of form 1 on host arrays of N emulated ranks (cost / idx [N][E]): the test hook. */
int f1p_comm_set_exchange(f1p_ctx* ctx, int32_t mode);
int f1p_argmin_gather_reduce_batch(f1p_ctx* ctx, const double* cost, const int32_t* idx, int32_t N, int32_t E, int32_t* idx_out, double* cost_out);
/* The two local steps of that exchange on host arrays (the collective in between is the caller's), so the key map can be
 * checked against np.argmin on a single GPU:  keys [E] <- key(cost);  masked_idx [E] <- idx where own_keys == min_keys
 * else INT32_MAX, cost_out [E] <- the cost min_keys encodes. */
int f1p_argmin_key_batch(f1p_ctx* ctx, const double* cost, int32_t E, uint64_t* keys);
int f1p_argmin_mask_batch(f1p_ctx* ctx, const uint64_t* own_keys, const uint64_t* min_keys, const int32_t* idx, int32_t E,
                          int32_t* masked_idx, double* cost_out);

#ifdef __cplusplus
}
#endif
#endif /* F1P_H */
