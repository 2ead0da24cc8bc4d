/*
 * dvo.h -- C ABI of libdvo.so: MI355X-native semi-dense direct visual odometry hot path.
 *
 * Drop-in boundary for the tracking/mapping path of KYabuuchi/direct-visual-odometry.  The reference has
 * no FFI/plugin layer (plain C++ classes over cv::Mat), so each entry point below names the C++ interface
 * it replaces (file:line under the reference tree).  All images are row-major contiguous float32, one
 * channel; gray in [0,1]; DVO_INVALID (-2.0f) marks unusable pixels (include/math/util.hpp:7-10); depth
 * and sigma in metres, depth 0 = none; K is a row-major 3x3; a twist xi is (vx,vy,vz,wx,wy,wz)
 * (src/math/se3.cpp:74-75); poses are row-major 4x4.
 *
 * Ownership: the caller owns every buffer it passes; the library copies on entry and never keeps a host
 * pointer.  `*_device` entry points take HIP device pointers (resident inputs, zero copy).
 * Errors: every call returns a dvo_status; nothing aborts or throws (the reference abort()s or throws
 * std::out_of_range: src/core/transform.cpp:16-17, include/system/frame.hpp:125).  Data sentinels are the
 * reference's: residual -1 and a zero update when no pixel is valid (src/track/optimize.cpp:92-93).
 * Threading: one handle = one HIP stream, used by one thread at a time; distinct handles are independent.
 */
#ifndef DVO_H
#define DVO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DVO_INVALID (-2.0f)
#define DVO_MAX_LEVELS 8
#define DVO_MAX_ITERATIONS 32

typedef enum {
    DVO_OK = 0,
    DVO_ERR_BAD_ARGUMENT = 1,
    DVO_ERR_HIP = 2,          /* a HIP runtime call failed; dvo_last_error() has the text            */
    DVO_ERR_NO_DEVICE = 3,    /* no gfx950 device visible: the library has NO CPU fallback            */
    DVO_ERR_NO_VALID_PIXELS = 4, /* informational: an optimize step had n_valid == 0                  */
    DVO_ERR_NOT_READY = 5,    /* e.g. track requested before a reference frame exists                 */
    DVO_ERR_OUT_OF_MEMORY = 6
} dvo_status;

/* Constants of the reference, runtime-configurable.  dvo_config_default() fills the reference's literals. */
typedef struct dvo_config {
    int      max_iterations;        /* 15    src/track/tracker.cpp:19                                   */
    float    min_update;            /* 5e-4  src/track/tracker.cpp:17                                   */
    float    min_residual;          /* 5e-3  src/track/tracker.cpp:16                                   */
    int      fixed_iterations;      /* 0 = early exit as the reference; N>0 = exactly N per level       */
    int      crop_enable;           /* 1 = level-2 crop of optimize.cpp:33-36 and mapper.cpp:90 crop    */
    float    step_default;          /* 2.0   src/track/optimize.cpp:22                                  */
    float    step_level1;           /* 1.5   src/track/optimize.cpp:23-24                               */
    float    step_level2;           /* 1.0   src/track/optimize.cpp:25-26                               */
    float    sigma_min, sigma_max;  /* 0.01, 0.5  src/track/optimize.cpp:83                             */
    float    min_depth;             /* 0.20  src/track/optimize.cpp:39                                  */
    float    keyframe_min_translation; /* 0.02 src/map/mapper.cpp:12                                    */
    int      keyframe_max_frames;   /* 6     src/map/mapper.cpp:13                                      */
    uint32_t rng_seed;              /* seed of the counter-based reset depth (replaces gaussian.cpp:8-9) */
    int      device;                /* HIP device ordinal                                                */
    void*    stream;                /* hipStream_t to launch on, or NULL for a library-owned stream      */
    int      profile;               /* 1 = bracket every k_track_gn launch with hipEvents (bench only)   */
    int      gn_pixels_per_thread;  /* 0 = choose from the problem size                                  */
    int      gn_use_lds_patch;      /* -1 = auto, 0 = global gathers, 1 = LDS-staged reference patch     */
    int      gn_gather_group;       /* 0 = auto; pixels per thread whose gathers are in flight together  */
    int      track_streams;         /* 0 = auto; sub-batches of a dvo_batch tracked on concurrent HIP streams */
    int      track_adaptive;        /* 0 = auto (on), -1 = off: the host stays two iterations ahead of the GPU and stops a level's launches once no sequence is active */
    int      track_fused_tiles;     /* N > 0: levels of at most N (<= 8) 1024-px tiles run all iterations in ONE launch; 0 = off (default) */
    int      track_single_launch;   /* 0 = auto: a dvo_vo handle's sensor-depth tracking runs in ONE launch per call (k_track_persist: co-resident workgroups,
                                       every wait bounded, falls back by itself); other handles of <= 8 sequences run one launch per Gauss-Newton
                                       iteration (the workgroup that finishes a sequence's last tile solves); 1 = one launch per iteration at most;
                                       -1 = launch pairs only.  Every setting gives the same bits at the same tile size */
} dvo_config;

void        dvo_config_default(dvo_config* cfg);
const char* dvo_version(void);
const char* dvo_status_string(int status);
const char* dvo_last_error(void);          /* thread-local text of the last failure */
int         dvo_device_count(void);        /* number of visible HIP devices (0 = none) */

/* ------------------------------------------------------------------------------------------------
 * System::VisualOdometry (include/system/system.hpp:12-104): frame in, pose out, one sequence.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dvo_vo dvo_vo;

/* VisualOdometry(const cv::Mat1f& K), system.hpp:15.  width/height = size of the frames that will be fed. */
int dvo_vo_create(const float K[9], int width, int height, const dvo_config* cfg, dvo_vo** out);
int dvo_vo_destroy(dvo_vo* vo);
/* Replaces the cv::randn initial depth of the first mono keyframe (include/system/frame.hpp:17-21):
 * depth/sigma at the culled base resolution (width/4 x height/4).  Optional; default = hash-based
 * N(1.5,0.5) clamped >= 0.5 with sigma 0.5. */
int dvo_vo_set_initial_depth(dvo_vo* vo, const float* depth, const float* sigma);
/* VisualOdometry(gray, depth, sigma, K), system.hpp:24-32: first keyframe with a given depth map. */
int dvo_vo_init_keyframe(dvo_vo* vo, const float* gray, const float* depth, const float* sigma);
/* cv::Mat1f odometrize(const cv::Mat1f& gray), system.hpp:44-74 -> 4x4 world pose exp(m_xi).
 * is_keyframe (optional) receives 1 when the frame was promoted to keyframe. */
int dvo_vo_odometrize(dvo_vo* vo, const float* gray, float T_world[16], int* is_keyframe);
/* the same fed with a raw u8 frame [height][width][channels] (channels 1 gray / 3 R,G,B / 4 R,G,B,A): cv::imread's output before
 * Loader::getNormalizedImages (src/core/loader.cpp:55-62); converted on the device, bit-identical to the float entry point */
int dvo_vo_odometrize_raw(dvo_vo* vo, const uint8_t* rgb, int channels, float T_world[16], int* is_keyframe);
/* cv::Mat1f odometrizeUsingDepth(gray, depth, sigma), system.hpp:77-93 -> 4x4 RELATIVE pose. */
int dvo_vo_odometrize_depth(dvo_vo* vo, const float* gray, const float* depth, const float* sigma, float T_rel[16]);
/* Lens undistortion of every mono frame (Loader::getNormalizedUndistortedImages, loader.cpp:15-42), fused into the pyramid build:
 * D = (k1, k2, p1, p2, k3) in OpenCV order, host memory, copied before the call returns; NULL clears.  Rules as
 * dvo_batch_set_distortion (one sequence, the K of dvo_vo_create): dvo_vo_odometrize and dvo_vo_odometrize_raw then give the bits a
 * plain handle gives fed dvo_op_undistort(frame, K, D), track log included.  Before the first frame only: after dvo_vo_odometrize*
 * or dvo_vo_init_keyframe -> DVO_ERR_NOT_READY, nothing changed (dvo_vo_load is not a frame and D is not stored: give a restored
 * handle its D again).  A handle with D set refuses dvo_vo_odometrize_depth, dvo_vo_odometrize_depth_raw and dvo_vo_init_keyframe
 * with DVO_ERR_BAD_ARGUMENT (sensor-depth frames are not undistorted). */
int dvo_vo_set_distortion(dvo_vo* vo, const float D[5]);
/* Photometric calibration of every raw mono frame (dvo_batch_set_photometric with one calibration and one sequence, same rules and
 * the same arithmetic): inv_response [256] or NULL (the default scale), vignette [height][width] or NULL (1); both NULL clears.
 * dvo_vo_odometrize_raw then gives the bits of a one-sequence calibrated mono batch, on the staged and the copied upload path alike.
 * Before the first frame only (-> DVO_ERR_NOT_READY after one, nothing changed; dvo_vo_load is not a frame and the calibration is
 * not stored: give a restored handle its calibration again); with or without dvo_vo_set_distortion, in either order.  Calibration needs the byte: a handle with a calibration refuses dvo_vo_odometrize and the sensor-depth entry points
 * (dvo_vo_odometrize_depth, dvo_vo_odometrize_depth_raw, dvo_vo_init_keyframe) with DVO_ERR_BAD_ARGUMENT. */
int dvo_vo_set_photometric(dvo_vo* vo, const float inv_response[256] /* or NULL */, const float* vignette /* [h][w] or NULL */);

/* FrameHistory (include/system/frame.hpp:146-188): keyframe / depth-map access. index 0 = oldest. */
int dvo_vo_keyframe_count(const dvo_vo* vo);
int dvo_vo_keyframe_info(const dvo_vo* vo, int index, int* id, int* levels, int* top_width, int* top_height,
                         float xi[6], float rel_xi[6]);
/* Frame::gray/depth/sigma/age/K at a pyramid level (frame.hpp:125-139); any output pointer may be NULL.
 * age is only stored for the top level. */
int dvo_vo_keyframe_get(const dvo_vo* vo, int index, int level, float* gray, float* depth, float* sigma,
                        float* age, float K[9]);
/* the most recent non-keyframe frame's pose (Frame::m_xi, m_relative_xi) */
int dvo_vo_last_frame_pose(const dvo_vo* vo, int* id, float xi[6], float rel_xi[6]);
int dvo_vo_last_valid_updates(const dvo_vo* vo); /* "valid update: N pixel", src/map/mapper.cpp:136 */

/* Per-iteration record the reference prints (src/track/tracker.cpp:56-61). */
typedef struct dvo_track_log {
    int   levels;
    int   n_iter[DVO_MAX_LEVELS];
    float residual[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    float update_norm[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    int   n_valid[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    float xi_after[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS][6];
    float xi_update[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS][6];  /* Outcome::xi_update of the iteration (optimize.cpp:98), before the composition */
} dvo_track_log;
int dvo_vo_last_track_log(const dvo_vo* vo, dvo_track_log* log);
/* Diagnostic (environment DVO_PERSIST_TIMELINE=1): wall-clock stamps (100 MHz) [2][64][8] the solver workgroup and worker 0 of the last
 * one-launch-per-call tracking kernel left per Gauss-Newton step (tools/persist_timeline.py prints them).  DVO_ERR_NOT_READY otherwise. */
int dvo_debug_persist_timeline(dvo_vo* vo, long long* out);

/* ------------------------------------------------------------------------------------------------
 * Batched tracking: n_seq independent sequences on one GPU, frame-to-frame with sensor depth
 * (the odometrizeUsingDepth loop of test/sequence.cpp:10-23, n_seq at a time).  Inputs are device
 * pointers to [n_seq][height][width] float32 arrays already resident in HBM.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dvo_batch dvo_batch;

int dvo_batch_create(int n_seq, const float K[9], int width, int height, int levels, int culls,
                     const dvo_config* cfg, dvo_batch** out);
int dvo_batch_destroy(dvo_batch* b);
/* Frame(gray,depth,sigma,K,levels,culls) for every sequence (frame.hpp:91-106): builds the pyramids of the
 * new frames, tracks them against the previous frames (Tracker::track, tracker.cpp:22-85) and makes them the
 * new reference.  The first call only stores the reference.  Asynchronous on the handle's stream.
 * NaN and +-inf in a pushed float map (every push entry point, dvo_vo_odometrize* included) are taken as the reference takes them
 * ("Non-finite pixels").  A cull (culls > 0, and every coarser level) reads through getPixel, which turns NaN
 * and -inf into DVO_INVALID and keeps +inf; at culls = 0 the finest level is a copy of the map.  Of what reaches a level:
 *   gray of the reference frame (sampled):   NaN, -inf are filled or gated like DVO_INVALID; +inf makes the sums NaN / inf: the
 *                                            solve answers NaN and the level is refused as below -- or, when no diagonal sum of H is
 *                                            > 0 (many such pixels), zero: "converged" with an infinite residual.
 *   gray of the tracked frame (per pixel):   -inf is gated out; NaN and +inf pass the gates (is_invalid is false for NaN): g and
 *                                            sum_r2 are not finite, every update of that level is refused (tracker.cpp:46-51) and the
 *                                            pose keeps the coarser levels' value.  ONE NaN gray pixel at a culls = 0 finest level
 *                                            freezes that level for the push: it runs max_iterations and the quality record shows
 *                                            DVO_QUALITY_NOT_FINITE | DVO_QUALITY_CAPPED, update_norm NaN, covariance NaN.
 *                                            With robust weights on (dvo_batch_set_robust_weights) the weight of a NaN or infinite
 *                                            residual is itself NaN by the formulas below, so H is poisoned too: no diagonal sum
 *                                            is > 0, the solve returns the ZERO update and the level ends after that iteration as
 *                                            DVO_QUALITY_CONVERGED with a NaN residual and without NOT_FINITE.
 *   depth of the reference:                  NaN, +-inf are gated out (as 0).
 *   sigma of the reference:                  +-inf are clamped to [sigma_min, sigma_max]; NaN poisons g like a NaN gray pixel.
 * Nothing else of the batch is affected: the other sequences' results keep their bits.  Consumers: INTEGRATION.md section 7. */
int dvo_batch_push_device(dvo_batch* b, const float* gray_dev, const float* depth_dev, const float* sigma_dev);
/* Optional look-ahead: build the pyramids of a frame that will be pushed later on a library-owned, low-priority side
 * stream, so that this HBM-bound pass runs beside the tracking of the frame pushed in between.  Call order per step:
 *   dvo_batch_prefetch_device(frame k+1); dvo_batch_push_device(frame k);
 * The same three pointers must later be handed to dvo_batch_push_device, in the order the frames were prefetched; at most
 * two may be waiting.  The buffers must be complete when this is called: the read is NOT ordered against the caller's
 * stream. */
int dvo_batch_prefetch_device(dvo_batch* b, const float* gray_dev, const float* depth_dev, const float* sigma_dev);
/* same, from host memory: the H2D copies run on a library-owned copy stream into one of two staging slots, so the transfer of
 * frame k+1 overlaps the tracking of frame k when the caller pushes without synchronising in between.  With PINNED host
 * buffers (hipHostMalloc / hipHostRegister) the copies are asynchronous: leave a buffer unchanged until a later
 * dvo_batch_synchronize / dvo_batch_last_poses.  A pageable buffer has been copied when the call returns (the call waits for the
 * copy, not for the tracking) and may be reused or freed at once. */
int dvo_batch_push_host(dvo_batch* b, const float* gray, const float* depth, const float* sigma);
/* The same three calls fed with RAW sensor frames, [n_seq][height][width] u8 gray / R,G,B / R,G,B,A (channels 1 / 3 / 4) + u16
 * depth: what cv::imread delivers before Loader::getNormalizedImages converts it (src/core/loader.cpp:137-147).  The conversion
 * (BGR2GRAY fixed-point luma, 1/255, depth * depth_scale [0 = 1/5000], sigma 0.1 / 1.0 and INVALID gray where depth == 0:
 * src/core/transform.cpp:60-76) runs inside the pyramid kernel on the pixels the pyramid keeps: 3 B/px (gray) instead of 12 B/px
 * cross PCIe and are read from HBM, and the results are bit-identical to dvo_op_ingest + the float entry points.  The HOST forms
 * (here, dvo_batch_odometrize_raw_host, dvo_vo_odometrize_raw, dvo_vo_odometrize_depth_raw) transfer only the image rows the pyramid
 * keeps -- every 2^culls-th, Convert::cullImage (src/core/convert.cpp:7-20) -- by one strided copy per buffer: half of the bytes
 * for Frame(g,d,s,K,4,1), a quarter for Frame(gray,K,3,2).  DVO_UPLOAD_FULL_FRAMES=1 in the environment restores whole frames. */
int dvo_batch_push_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels, const uint16_t* depth16_dev, float depth_scale);
int dvo_batch_prefetch_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels, const uint16_t* depth16_dev, float depth_scale);
int dvo_batch_push_raw_host(dvo_batch* b, const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale);
/* relative twists [n_seq][6] and 4x4 relative poses [n_seq][16] of the last push (synchronises). NULL = skip */
int dvo_batch_last_poses(dvo_batch* b, float* xi_rel, float* T_rel);
/* asynchronous device-to-device copy of the last push's poses (on the handle's stream): pose-out without a
 * host round trip.  xi_dst_dev [n_seq][6], T_dst_dev [n_seq][16]; either may be NULL. */
int dvo_batch_copy_poses_device(dvo_batch* b, float* xi_dst_dev, float* T_dst_dev);
int dvo_batch_last_track_log(dvo_batch* b, int seq, dvo_track_log* log);
int dvo_batch_synchronize(dvo_batch* b);
/* gray and depth [h][w] of pyramid level `level` (0 = coarsest) of the frame the last push gave sequence `seq` = the reference of the
 * next push (synchronises); either pointer may be NULL.  DVO_ERR_NOT_READY before the first push.  With keyframe tracking the
 * references are the keyframes (dvo_batch_keyframe_get) and this returns the frame of the last push, the one it tracked (a SKIPPED
 * sequence's slot holds a copy of its keyframe as it was before the push). */
int dvo_batch_frame_get(dvo_batch* b, int seq, int level, float* gray, float* depth);
/* Diagnostic, read-only: how the Gauss-Newton launches of pyramid level `level` (0 = coarsest) are planned for the NEXT push / call of a
 * sensor-depth or mono batch, with the opt-in terms (robust weights, affine brightness, geometric) as they are set now: pixels per
 * thread and gather group (the kernel instance: cfg.gn_pixels_per_thread = 0 lets the engine choose per level), whether the level
 * runs the 2-D tiles, the tiles (partial rows) per sequence, and the launch form.  Launches nothing, changes nothing; any output may
 * be NULL.  DVO_ERR_BAD_ARGUMENT for a NULL handle or a level outside the pyramid.  The tests name the instance they ran from this. */
#define DVO_PLAN_PAIRS     0   /* one accumulation and one solve launch per iteration, the global-gather kernel (every opt-in term) */
#define DVO_PLAN_ITERATION 1   /* one launch per iteration (small plain handles); launch pairs where that launch is refused */
#define DVO_PLAN_LEVEL     2   /* one launch per level (cfg.track_fused_tiles) */
#define DVO_PLAN_LDS_PATCH 3   /* launch pairs of the LDS-patch kernel (cfg.gn_use_lds_patch > 0) */
int dvo_debug_batch_level_plan(dvo_batch* b, int level, int* ppt, int* group, int* tiles_2d, int* tiles, int* schedule);
/* ---- per-sequence skip and restart (sensor-depth batches) -------------------------------------------------------------------
 * dvo_batch_set_actions gives every sequence an action for the NEXT push (any of dvo_batch_push_device / _host / _raw_device /
 * _raw_host); afterwards the actions are spent.  actions[n_seq]: host memory (actions_on_device = 0) is copied before the call
 * returns; device memory (actions_on_device = 1) is read in stream order on the handle's stream when that push runs, under the
 * same rule as the push_device inputs (so actions can be computed on the GPU, e.g. from the previous poses).  NULL clears them.
 *   SKIP     the sequence's input slot is never read (it may hold anything); its reference stays the frame it had; its relative
 *            pose is the zero twist / identity T and its track log has n_iter = 0 on every level.  A SKIP on a sequence with no
 *            reference leaves it without one.
 *   TRACK    as a plain push, bit for bit: track against the sequence's reference, then the frame becomes the reference.
 *            On a sequence with no reference yet it acts as RESTART.
 *   RESTART  forget the reference: the frame is the sequence's first frame (system.hpp:83-86), pose zero / identity.
 * Whether a sequence has a reference is per-sequence device state, empty after dvo_batch_create.  A batch that never sets
 * actions runs exactly the launches it always ran; dvo_batch_last_status then reports all STARTED after the first push and
 * all TRACKED after later ones.  Once a batch has used actions, a push without dvo_batch_set_actions is an all-TRACK push of
 * the per-sequence path (a sequence skipped from the start then reports STARTED), and every such push has poses
 * (dvo_batch_last_poses), even one in which no sequence tracked.
 * Errors, returned before anything is enqueued: a mono batch or a NULL handle -> DVO_ERR_BAD_ARGUMENT; actions together with
 * prefetch are not supported: set_actions while a prefetched frame waits, or dvo_batch_prefetch_* while actions are pending ->
 * DVO_ERR_NOT_READY; a push with actions whose weight storage differs from the current references' (float maps after raw frames
 * or the reverse) -> DVO_ERR_BAD_ARGUMENT.  Mono batches (dvo_batch_create_mono) refuse these three calls: they take
 * dvo_batch_set_mono_actions (below). */
#define DVO_SEQ_SKIP    0   /* no frame for this sequence this step: input slot NOT read, reference kept */
#define DVO_SEQ_TRACK   1   /* as today: track against the sequence's reference, then the frame becomes the reference */
#define DVO_SEQ_RESTART 2   /* forget the reference: the frame is the sequence's first frame (system.hpp:83-86) */
/* per-sequence outcome of the last push */
#define DVO_SEQ_TRACKED    0
#define DVO_SEQ_SKIPPED    1
#define DVO_SEQ_STARTED    2   /* RESTART, or TRACK on a sequence that had no reference yet */
#define DVO_SEQ_BAD_ACTION 3   /* action value not in {0,1,2}: handled as SKIP */
int dvo_batch_set_actions(dvo_batch* b, const uint8_t* actions, int actions_on_device);   /* [n_seq]; NULL clears */
int dvo_batch_last_status(dvo_batch* b, int* status);             /* [n_seq], host, synchronises; DVO_ERR_NOT_READY before the first push */
int dvo_batch_copy_status_device(dvo_batch* b, int* status_dev);  /* [n_seq], async device-to-device copy on the handle's stream */
/* ---- per-sequence camera intrinsics (sensor-depth batches) ------------------------------------------------------------------
 * dvo_batch_set_intrinsics gives every sequence its own K: K[n_seq][9], host memory, row-major 3x3 (fx = K[0], cx = K[2],
 * fy = K[4], cy = K[5]), copied before the call returns; NULL puts every sequence back on the K of dvo_batch_create.  The table
 * takes effect at the NEXT push (any of the four push entry points) and stays in force after it.  The frame size, pyramid shape,
 * configuration and raw depth_scale stay per handle.  Each level's intrinsics are derived from K exactly as dvo_batch_create
 * derives them, so a sequence tracks bit for bit as a one-sequence batch created with its K would.
 * Camera-change rule: a reference frame belongs to the camera it was taken with.  A sequence whose fx, fy, cx or cy differ (in
 * bits) at a push from the table of the previous push loses its reference at that push, before its action is resolved:
 *   TRACK (or no actions)  starts instead: status DVO_SEQ_STARTED, zero twist, identity T; the frame becomes its reference
 *   SKIP / bad action      reported as usual (SKIPPED / BAD_ACTION); the sequence is left without a reference
 *   RESTART                unchanged
 * Once intrinsics have been set, every push runs the per-sequence path (as after dvo_batch_set_actions); a batch that never sets
 * them runs exactly the launches it always ran.  dvo_batch_probe_gn keeps using the creation K.
 * Errors, returned before anything is enqueued: a mono batch, a NULL handle, or a K with a non-finite entry or fx / fy <= 0 ->
 * DVO_ERR_BAD_ARGUMENT; a prefetched frame waiting for its push -> DVO_ERR_NOT_READY.
 * dvo_batch_get_intrinsics copies the table the next push uses ([n_seq][9], host, synchronous): the creation K until set. */
int dvo_batch_set_intrinsics(dvo_batch* b, const float* K);   /* [n_seq][9]; NULL = the creation K for every sequence */
int dvo_batch_get_intrinsics(dvo_batch* b, float* K);         /* [n_seq][9] */
/* ---- lens undistortion of sensor-depth frames (RGB-D cameras) -------------------------------------------------------------
 * dvo_batch_set_sensor_distortion undistorts every frame of a sensor-depth batch (dvo_batch_create) while its pyramid is built:
 * D = [5] for every sequence (per_sequence = 0) or [n_seq][5] (per_sequence = 1), OpenCV order (k1, k2, p1, p2, k3), host memory,
 * copied before the call returns.  NULL clears.  Applies from the NEXT push on (any push or prefetch entry point, float or raw,
 * device or host): sequence s then gives, bit for bit, the poses, status and track log a plain batch with the same creation K,
 * intrinsics table, config, actions and feeds gives when it is fed dvo_op_undistort(m, K_s, D_s) of each of gray, depth and sigma
 * (raw frames: of each of the three maps dvo_op_ingest returns).
 *  - The undistortion camera of s is its CURRENT full-resolution K: the creation K, or row s of the dvo_batch_set_intrinsics table in
 *    force at that push.  The new camera matrix is that same K (initUndistortRectifyMap(K, D, I, K)), nearest neighbour: depth is
 *    z-depth and is never interpolated.  Outside the image all three maps are DVO_INVALID (such a pixel never contributes).
 *  - An all-zero D row is still applied: it gives what dvo_op_undistort gives with zero D (a mixed rig marks an undistorted camera so).
 *  - Camera-change rule: a sequence's camera is (fx, fy, cx, cy, D or none).  A sequence whose D changes in bits at a push, or goes
 *    between none and a row, loses its reference there exactly as for a change of K (see dvo_batch_set_intrinsics).
 *  - Before the first push the call only selects the kernel: a batch that sets D there and no actions or intrinsics stays on the
 *    plain path.  After it, the batch runs the per-sequence path from then on, as after dvo_batch_set_intrinsics.
 *  - The remap is computed here (one table of int32 source indices per distinct (fx, fy, cx, cy, D), (width >> culls) x
 *    (height >> culls) entries: 307 KB at 640x480, cull 1) and gathered inside the pyramid kernel: no undistorted frame is stored.
 *    The host entry points then upload whole frames instead of the rows the pyramid keeps.
 *  - SYNCHRONOUS: this call, and dvo_batch_set_intrinsics while D is set and a sequence's K changes, wait for the work queued on the
 *    handle's stream before they replace the tables (camera swaps are rare).  Pushes queued before the call give the same results.
 *  - Errors, returned before anything changes: a NULL handle, a non-finite coefficient (dvo_last_error names the first bad
 *    sequence) or a mono batch (use dvo_batch_set_distortion) -> DVO_ERR_BAD_ARGUMENT; a prefetched frame waiting for its push ->
 *    DVO_ERR_NOT_READY.
 * A batch that never sets D runs exactly the kernels it runs without this call.  The single-stream dvo_vo depth entry points do not
 * undistort (a one-sequence batch does).
 * get: the D the next push uses, [n_seq][5] (zeros when none; may be NULL), and *enabled = 1 when set (may be NULL). */
int dvo_batch_set_sensor_distortion(dvo_batch* b, const float* D, int per_sequence);
int dvo_batch_get_sensor_distortion(dvo_batch* b, float* D /*[n_seq][5], may be NULL*/, int* enabled /*may be NULL*/);
/* ---- low-pass filtered gray pyramid of sensor-depth frames (opt-in) ---------------------------------------------------------
 * By default every pyramid level is a decimation (level l holds pixel (x << s, y << s) of the input), so a coarse level carries
 * the full per-pixel noise of the source.  dvo_batch_set_pyramid_filter(b, DVO_PYRAMID_FILTER_BINOMIAL3) makes every push and
 * prefetch of a sensor-depth batch (dvo_batch_create; float or raw, device or host) build its GRAY pyramid with a 3x3 binomial
 * filter before each halving.  Depth, sigma and the weight maps of every level stay the plain build's, bit for bit, and
 * everything downstream (actions, cameras, keyframes, fusion, carry, export, every opt-in term) reads the frame sets as before.
 * Contract (all arithmetic float32, IEEE, no contraction but the fmaf named):
 *  - G0 is the converted source gray at input resolution (never stored): for raw frames the gray of the raw conversion (see
 *    dvo_op_pyramid_frames), DVO_INVALID where d16 == 0; for float feeds the float map.
 *  - A pixel is invalid if it is NaN or <= DVO_INVALID.
 *  - One halving H of a w_in x h_in map gives, for 0 <= x < w_in >> 1 and 0 <= y < h_in >> 1: DVO_INVALID if the centre tap
 *    G(2x, 2y) is invalid; else S = 0.0f, W = 0, and for j = -1, 0, 1 (outer) and i = -1, 0, 1 (inner), skipping a tap
 *    (2x + i, 2y + j) that is outside the map or invalid: k = (2 - |i|)(2 - |j|), S = fmaf((float)k, g, S), W += k; the result is
 *    S / (float)W, one IEEE division.
 *  - The top-level gray is H applied `culls` times to G0 (culls = 0: the input unchanged, as without the filter); the gray of level
 *    l - 1 is H of the STORED level l.
 *  - So the valid set of every level equals the plain build's, and below an unchanged top no result is NaN.
 *  - A DVO_SEQ_SKIP sequence copies its reference's gray forward level by level.
 * The host entry points upload whole frames while the filter is on, and the split build of big batches is not used.
 * The filter is fixed once the handle has seen a frame: the setter succeeds before the first push or prefetch, afterwards only
 * with the value in force.  DVO_ERR_BAD_ARGUMENT, before anything is queued: a NULL handle or out pointer, a value outside the
 * set, a mono batch, another value after the first frame, a batch with dvo_batch_set_sensor_distortion on
 * (dvo_batch_set_sensor_distortion refuses likewise while the filter is on), a batch created with culls > 2.
 * Out of scope: mono batches, the dvo_vo handles, the combination with lens undistortion.
 * A batch that never calls the setter, or sets NONE, runs exactly the launches it runs without this call. */
#define DVO_PYRAMID_FILTER_NONE      0
#define DVO_PYRAMID_FILTER_BINOMIAL3 1
int dvo_batch_set_pyramid_filter(dvo_batch* b, int filter);   /* sensor-depth batches */
int dvo_batch_pyramid_filter(dvo_batch* b, int* filter);
/* ---- one block of sequences per GPU (BASELINE config 5) -------------------------------------------
 * The path shards across sequences only (frame t of a sequence tracks against state from frames < t: system.hpp:48,57,67): every
 * rank -- one process per GPU -- owns a contiguous block of the sequences and tracks it with no communication.
 * dvo_shard_range: the block of `rank` (counts differ by at most one; the split of dvo_amd/shard.py and bench.py --gpus N).
 * dvo_batch_gather_poses_rccl: the one collective of the path, from C++: an all-gather of the last push's twists over RCCL / xGMI,
 * queued on the handle's stream.  `rccl_comm` is the caller's ncclComm_t (ncclCommInitRank over its own bootstrap -- MPI,
 * torch.distributed's store, a shared file); every rank must hold the same n_seq (pad the last block).  xi_all_dev: device memory
 * [world_size][n_seq][6].  librccl.so is loaded on first use (dlopen): DVO_ERR_NOT_READY with an explanation when it is absent. */
int dvo_shard_range(int n_sequences, int world_size, int rank, int* first, int* count);
int dvo_batch_gather_poses_rccl(dvo_batch* b, void* rccl_comm, int world_size, float* xi_all_dev);
/* Profile counters (cfg.profile = 1): accumulated over every k_track_gn launch since the last reset. */
typedef struct dvo_gn_profile {
    double   gn_ms;             /* sum of hipEvent-bracketed k_track_gn durations                         */
    uint64_t gn_launches;
    uint64_t gn_pixels;         /* pixels evaluated (active sequences x level pixels), summed              */
    uint64_t gn_iterations;     /* sequence-iterations executed                                            */
} dvo_gn_profile;
int dvo_batch_profile(dvo_batch* b, dvo_gn_profile* out, int reset);
/* Roofline probe: launch k_track_gn `n_launches` times back to back on level `level` with every sequence
 * active (poses unchanged, partials discarded) and return the average duration from two hipEvents. */
int dvo_batch_probe_gn(dvo_batch* b, int level, int n_launches, float* avg_ms, uint64_t* pixels_per_launch);

/* ------------------------------------------------------------------------------------------------
 * Batched MONO pipeline: System::VisualOdometry::odometrize (system.hpp:44-74) = Tracker::track against the newest keyframe +
 * Map::Mapper::estimate / regularize (src/map/mapper.cpp:16-144), n_seq sequences per call.  The keyframe decision
 * (Mapper::needNewFrame, mapper.cpp:45-60) is taken per sequence ON THE DEVICE; one call enqueues a fixed launch sequence and
 * returns.  FrameHistory (include/system/frame.hpp:146-188) is a ring of the newest `ring_keyframes` keyframes per sequence.
 * Every sequence gives the bits a dvo_vo handle with the same config gives (and, past `ring_keyframes` keyframes, one with
 * dvo_vo_set_history_limit(ring_keyframes)).
 * ------------------------------------------------------------------------------------------------ */
int dvo_batch_create_mono(int n_seq, const float K[9], int width, int height, int ring_keyframes, const dvo_config* cfg, dvo_batch** out);
/* The same with one K per sequence: K[n_seq][9], host memory, row-major 3x3 (fx = K[0], cx = K[2], fy = K[4], cy = K[5]), copied
 * before the call returns.  Same arguments and results as dvo_batch_create_mono otherwise, and every other mono entry point works
 * unchanged on the handle.  A sequence's K is fixed at creation: its keyframe ring and depth maps belong to that camera (a restart,
 * dvo_batch_set_mono_actions, keeps it; dvo_batch_set_intrinsics, dvo_batch_get_intrinsics and dvo_batch_set_actions refuse a mono batch).  Each sequence
 * gives the bits a dvo_vo handle created with that sequence's K and the same config gives (past `ring_keyframes` keyframes, one with
 * dvo_vo_set_history_limit(ring_keyframes)).  Frame size, pyramid shape and config stay per handle.
 * Errors, returned before anything touches the GPU: K == NULL, or a sequence's K with a non-finite entry or fx / fy <= 0 ->
 * DVO_ERR_BAD_ARGUMENT, with the index of the first bad sequence in dvo_last_error. */
int dvo_batch_create_mono_cameras(int n_seq, const float* K /*[n_seq][9]*/, int width, int height, int ring_keyframes,
                                  const dvo_config* cfg, dvo_batch** out);
/* Initial depth / sigma of the first keyframes (replaces cv::randn, frame.hpp:17-21) at width/4 x height/4: one host map for every
 * sequence, or device maps [n_seq][height/4][width/4].  Optional; default as dvo_vo. Call before the first frame. */
int dvo_batch_set_initial_depth(dvo_batch* b, const float* depth, const float* sigma);
int dvo_batch_set_initial_depth_device(dvo_batch* b, const float* depth_dev, const float* sigma_dev);
/* odometrize(gray) for every sequence: gray_dev = [n_seq][height][width] float32 in HBM.  Asynchronous on the handle's stream. */
int dvo_batch_odometrize_device(dvo_batch* b, const float* gray_dev);
/* same from raw u8 frames [n_seq][height][width][channels] (channels 1 / 3 / 4), converted inside the pyramid kernel */
int dvo_batch_odometrize_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels);
/* the same two from host memory (copy stream + two staging slots, as dvo_batch_push_host) */
int dvo_batch_odometrize_host(dvo_batch* b, const float* gray);
int dvo_batch_odometrize_raw_host(dvo_batch* b, const uint8_t* rgb, int channels);
/* world twists [n_seq][6], world poses exp(xi) [n_seq][16] (system.hpp:73) and keyframe flags [n_seq] of the last frame
 * (synchronises); any pointer may be NULL.  _device: asynchronous device-to-device copies on the handle's stream.  These two and
 * dvo_batch_keyframe_get also serve a sensor-depth batch with keyframe tracking (dvo_batch_set_keyframe_tracking, below). */
int dvo_batch_world_poses(dvo_batch* b, float* xi_world, float* T_world, int* is_keyframe);
int dvo_batch_copy_world_poses_device(dvo_batch* b, float* xi_dst_dev, float* T_dst_dev, int* key_dst_dev);
/* the newest keyframe of sequence `seq` (FrameHistory::getRefFrame, frame.hpp:159-166): maps of one pyramid level (age: top level
 * only), its world twist, id, the number of keyframes the sequence has created and the valid-update count of the last frame */
int dvo_batch_keyframe_get(dvo_batch* b, int seq, int level, float* gray, float* depth, float* sigma, float* age, float xi[6], int* id,
                           int* n_keyframes, int* valid_updates);
/* Lens undistortion of every frame of a mono batch (Loader::getNormalizedUndistortedImages, loader.cpp:15-42; main.cpp:44-49 feeds
 * its output to odometrize): D = [5] for every sequence (per_sequence = 0) or [n_seq][5] (per_sequence = 1), OpenCV order
 * (k1, k2, p1, p2, k3), host memory, copied before the call returns.  NULL clears.  From then on every frame that enters through
 * any odometrize entry point -- float or raw, device or host -- is undistorted first: sequence s gives, bit for bit, the world poses,
 * keyframe flags, keyframe maps and mono stats a plain handle with the same K, config and initial depth gives when it is fed
 * dvo_op_undistort(frame_s, K_s, D_s) (raw frames: of their dvo_op_ingest gray).
 *  - The undistortion K of a sequence is its creation K at full resolution: the K of dvo_batch_create_mono, or row s of
 *    dvo_batch_create_mono_cameras.  The new camera matrix is that same K (initUndistortRectifyMap(K, D, I, K)), nearest
 *    neighbour, DVO_INVALID outside the image.
 *  - An all-zero D is still applied: it gives what dvo_op_undistort gives with zero D.
 *  - The remap is computed once here (one table of int32 source indices per distinct (K, D), (width/4) x (height/4) entries) and
 *    gathered inside the pyramid kernel: no undistorted frame is stored.  The host entry points then upload whole frames instead of
 *    the one row in four the pyramid keeps (4x the PCIe bytes).
 *  - Errors, returned before anything is enqueued: a NULL handle, a non-finite coefficient (dvo_last_error names the first bad
 *    sequence) or a sensor-depth batch (dvo_batch_create) -> DVO_ERR_BAD_ARGUMENT; a call after the batch has consumed a frame
 *    -> DVO_ERR_NOT_READY, nothing changed (D is fixed for the life of the keyframes, as K).
 * A batch that never sets D runs exactly the kernels it runs without this call.
 * get: D [n_seq][5] as set (zeros when none; may be NULL) and *enabled = 1 when set (may be NULL). */
int dvo_batch_set_distortion(dvo_batch* b, const float* D, int per_sequence);
int dvo_batch_get_distortion(dvo_batch* b, float* D /*[n_seq][5]*/, int* enabled);
/* Photometric calibration of every raw frame of a mono batch: the camera's inverse response (a 256-entry table) and its vignette
 * (a per-pixel attenuation map), the TUM monoVO convention (pcalib.txt, vignette.png), applied inside the pyramid kernel where each
 * kept pixel is touched once, as a byte.  n_cal calibrations and, per sequence, which one it uses; host memory, copied before the call
 * returns.  n_cal = 0 clears it; both arrays NULL with n_cal = 0 is the only way to turn it off.
 * For every pixel the library keeps from a raw frame of sequence s with calibration c = seq_cal[s]:
 *     g8   = the byte (1 channel) or the fixed-point luma of dvo_op_ingest (3 / 4 channels)          -- unchanged
 *     p    = the frame's own pixel this kept pixel comes from: (x << 2, y << 2) without D, the remap table's source index with D
 *            (index -1 stays DVO_INVALID)
 *     gray = inv_response[c][g8] * (1.0f / vignette[c][p])    -- float32: one IEEE division (done once, at set time), one multiply,
 *            no contraction
 *     gray = DVO_INVALID  where vignette[c][p] is not finite or <= 0
 *  - inv_response is in the library's gray units ([0, 1]).  NULL means (float)i * (float)(1.0 / 255.0), which is dvo_op_ingest's scale.
 *  - vignette NULL means 1.  A denormal entry is positive and finite: its gain is +inf, and the product is what IEEE gives (inf, or
 *    NaN for a zero response), which every consumer treats as it treats such a value in a float frame.
 *  - With a multi-channel frame the response is applied to the luma, not per channel.
 *  - Everything downstream is the existing pipeline on that gray: sequence s gives, bit for bit, the world poses, keyframe flags,
 *    keyframe maps and mono stats of a plain handle fed the float frames `gray` above.
 *  - A non-positive vignette entry doubles as a static per-camera mask (a bonnet, a lens hood): the pixel is DVO_INVALID in every
 *    frame of the sequence, so it is neither tracked on nor mapped.
 *  - Exposure times are not part of it: a known per-frame exposure is a gain, which dvo_batch_set_affine_rows in GIVEN mode takes.
 *  - Before the first frame only: a call after the batch has consumed a frame -> DVO_ERR_NOT_READY, nothing changed.
 *  - DVO_ERR_BAD_ARGUMENT, nothing changed: a NULL handle, a sensor-depth batch, n_cal < 0, both arrays NULL with n_cal > 0, an index
 *    outside [0, n_cal), or a response entry that is not finite or is negative.  dvo_last_error names the first bad calibration or
 *    sequence.
 *  - It works with or without dvo_batch_set_distortion, set in either order: the tables that result are the same (one float table
 *    of gains per distinct (calibration, undistortion camera) pair at top-level resolution, (width/4) x (height/4), indexed by the
 *    kept pixel; without D the host entry points keep uploading only the rows the pyramid keeps).
 *  - Calibration needs the byte: on a handle with a calibration the float-feed entry points (dvo_batch_odometrize_device,
 *    dvo_batch_odometrize_host) return DVO_ERR_BAD_ARGUMENT.
 *  - SKIP / RESTART plans, per-sequence cameras, pose guesses, robust weights, affine brightness and track quality need no knowledge
 *    of it.  A batch that never calls the setter runs exactly the launches it runs without this entry point.
 * get: *n_cal (0 when none; may be NULL) and seq_cal [n_seq] as set (zeros when none; may be NULL). */
int dvo_batch_set_photometric(dvo_batch* b, int n_cal, const float* inv_response /* [n_cal][256], or NULL */,
                              const float* vignette /* [n_cal][height][width], or NULL */,
                              const int* seq_cal /* [n_seq] in [0, n_cal), or NULL = 0 for every sequence */);
int dvo_batch_get_photometric(dvo_batch* b, int* n_cal, int* seq_cal /* [n_seq], may be NULL */);
/* Per-sequence counters of a mono batch.  `clamped_pixels` makes the one deviation of the ring from the reference's unbounded
 * FrameHistory (frame.hpp:146-188) visible: a pixel older than the `ring_keyframes` retained keyframes is searched against the
 * oldest retained one instead of the keyframe it was born in (mapper.cpp:99-101, frame_history[age]); the count is cumulative and
 * stays 0 until a sequence has created more than `ring_keyframes` keyframes AND a pixel has survived all of them. */
typedef struct dvo_mono_stats {
    int frames;                    /* frames consumed (Frame::latest_id + 1) */
    int keyframes_created;
    int ring_keyframes;
    int valid_updates_last_frame;  /* mapper.cpp:136 */
    int clamped_pixels;
} dvo_mono_stats;
int dvo_batch_mono_stats(dvo_batch* b, int seq, dvo_mono_stats* out);
/* ---- per-sequence skip / restart of a mono batch ------------------------------------------------------------------------------
 * dvo_batch_set_mono_actions: actions[n_seq] (DVO_SEQ_SKIP / TRACK / RESTART) for the NEXT mono call (any dvo_batch_odometrize_*
 * entry point); spent afterwards.  Host memory (actions_on_device = 0) is copied before the call returns; device memory
 * (actions_on_device = 1) is read in stream order when that call runs.  NULL clears them.  Each sequence holds one piece of device
 * state, "has a keyframe", empty at creation.
 *   SKIP     the input slot is never read (it may hold NaN or garbage) and nothing of the sequence changes: keyframe ring, maps,
 *            frame counter, stats.  Its world pose keeps the value of its last consumed frame (zero twist / identity if it never
 *            started), is_keyframe = 0, track log n_iter = 0 on every level.  Status DVO_SEQ_SKIPPED.
 *   TRACK    odometrize as a plain call.  On a sequence without a keyframe it acts as RESTART.  Status DVO_SEQ_TRACKED.
 *   RESTART  the frame becomes the sequence's frame 0 (system.hpp:49-54): first keyframe, identity pose, is_keyframe = 1, the ring
 *            emptied, frame ids counted from 0 again, age 0, depth and sigma from the start map.  Status DVO_SEQ_STARTED.
 *   other    handled as SKIP.  Status DVO_SEQ_BAD_ACTION.
 * Cut a sequence's calls at every start: each segment gives, bit for bit, what a fresh dvo_vo handle with the sequence's K (and D),
 * the same config, dvo_vo_set_history_limit(ring_keyframes) and the segment's start map gives on the frames the sequence consumed.
 * Start map of a start, the first rule that applies: (1) row s of dvo_batch_set_mono_start_depth_device, if set for this call;
 * (2) on a sequence's first start only, the map its slot was given before the first call (dvo_batch_set_initial_depth,
 * dvo_batch_set_initial_depth_device, or the default); (3) the host map of dvo_batch_set_initial_depth, if one was given;
 * (4) the default map (the one dvo_vo uses).
 * Once a batch has used actions, every later call runs the per-sequence path and a call without actions is an all-TRACK call.  A
 * batch that never sets actions runs exactly the launches it always ran; its status is all STARTED after the first call and all
 * TRACKED after later ones.  dvo_batch_keyframe_get and dvo_batch_mono_stats (frames = frames since the sequence's last start)
 * return DVO_ERR_NOT_READY for a sequence that never started; dvo_batch_world_poses works after the first call.  K and D stay those
 * of the handle.  A call that fails consumes no frame and spends neither actions nor start maps.
 * Errors, returned before anything is enqueued: a NULL handle or a sensor-depth batch -> DVO_ERR_BAD_ARGUMENT (dvo_batch_set_actions,
 * dvo_batch_last_status and dvo_batch_copy_status_device keep refusing mono batches).
 * dvo_batch_mono_last_status: [n_seq], host, synchronises; DVO_ERR_NOT_READY before the first call.
 * dvo_batch_copy_mono_status_device: [n_seq], asynchronous device-to-device copy on the handle's stream.
 * dvo_batch_set_mono_start_depth_device: start maps [n_seq][height/4][width/4] in device memory, read in stream order at the NEXT call
 * and only for the sequences that start in it; spent afterwards.  NULL, NULL clears them; exactly one NULL -> DVO_ERR_BAD_ARGUMENT. */
int dvo_batch_set_mono_actions(dvo_batch* b, const uint8_t* actions, int actions_on_device);
int dvo_batch_mono_last_status(dvo_batch* b, int* status);
int dvo_batch_copy_mono_status_device(dvo_batch* b, int* status_dev);
int dvo_batch_set_mono_start_depth_device(dvo_batch* b, const float* depth_dev, const float* sigma_dev);
/* ---- per-sequence start pose of the tracking (both batch kinds) ----------------------------------------------------------------
 * Every frame's Gauss-Newton starts from the zero twist (tracker.cpp:28).  dvo_batch_set_pose_guess_mode picks, per handle, where
 * level 0's first iteration of each TRACK sequence starts instead; it takes effect at the next push / call and stays set.  The stop
 * rules, iteration caps, track log, the meaning of the returned poses, keyframe decisions and mapping are unchanged.
 *   DVO_GUESS_NONE              zero (tracker.cpp:28): what a batch that never sets a mode does (the same bits).
 *   DVO_GUESS_GIVEN             the rows of dvo_batch_set_pose_guess, in the convention of what the batch returns: the relative
 *                               twist of the frame being pushed as dvo_batch_last_poses returns it (sensor depth), or the frame's
 *                               world twist g as dvo_batch_world_poses returns it (mono: the tracker starts from
 *                               se3_concatenate(-ref_xi, g), ref_xi = the sequence's current keyframe twist).  Rows are spent by
 *                               the next push / call; one without rows starts from zero.
 *   DVO_GUESS_CONSTANT_VELOCITY computed on the device.  Sensor depth: the relative twist of the sequence's most recent TRACKED push
 *                               since its last start (zero after STARTED / RESTART or a camera or distortion change; SKIP keeps
 *                               it).  Mono: with w1, w2 the world twists returned for the sequence's last two calls that tracked or
 *                               started it since its last start, g = concatenate(w1, concatenate(-w2, w1)) and the start is
 *                               concatenate(-ref_xi, g); zero while only w1 exists.  concatenate is dvo_op_se3_concatenate's
 *                               float function.  The history is kept from the first push after the first mode was set.
 * dvo_batch_set_pose_guess: xi[n_seq][6].  Host rows (xi_on_device = 0) are copied before the call returns; device rows are read in
 * stream order on the handle's stream when the next push runs (as dvo_batch_set_actions).  Rows of sequences that do not TRACK are
 * never read (they may hold NaN); a TRACK row with a non-finite entry starts from zero.  NULL clears pending rows.
 * dvo_batch_last_start_poses: [n_seq][6] the twist each TRACKED sequence started from at the last push (zeros for the others and in
 * DVO_GUESS_NONE); host, synchronises; DVO_ERR_NOT_READY before the first push.
 * Errors, returned before anything is enqueued: a NULL handle, a mode outside {0, 1, 2}, or rows while the mode is not
 * DVO_GUESS_GIVEN -> DVO_ERR_BAD_ARGUMENT.  dvo_vo handles have no guess. */
#define DVO_GUESS_NONE              0
#define DVO_GUESS_GIVEN             1
#define DVO_GUESS_CONSTANT_VELOCITY 2
int dvo_batch_set_pose_guess_mode(dvo_batch* b, int mode);
int dvo_batch_set_pose_guess(dvo_batch* b, const float* xi, int xi_on_device);
int dvo_batch_last_start_poses(dvo_batch* b, float* xi_start);
/* ---- keyframe tracking of a sensor-depth batch --------------------------------------------------------------------------------
 * A sensor-depth batch tracks frame to frame (odometrizeUsingDepth, system.hpp:77-93): every frame's tracking error stays in the
 * trajectory.  dvo_batch_set_keyframe_tracking(b, 1) makes it track each frame against a retained KEYFRAME of its sequence instead,
 * replaced only when the mono rule fires (Mapper::needNewFrame, mapper.cpp:45-60: |t| of the twist against the keyframe >
 * cfg.keyframe_min_translation, or cfg.keyframe_max_frames frames since it), decided per sequence on the device with the mono batch's
 * own function (the same bits).  enable = 0 puts the handle back on frame-to-frame tracking.  Per sequence and push:
 *   start    (the first push, RESTART, TRACK without a keyframe, a change of K or D: as dvo_batch_set_actions resolves them) the frame
 *            becomes the keyframe; world pose identity, frame counter 0, is_keyframe = 1; status DVO_SEQ_STARTED.
 *   TRACK    the frame is tracked against the keyframe (from zero or the pose guess).  Frame id = the previous one + 1 (skipped pushes
 *            do not count); world twist = se3_concatenate(keyframe twist, relative twist), as the mono batch (frame.cpp:7-14);
 *            is_keyframe = the rule, and when it fires the frame's pyramid (gray, depth and, where stored, the weight maps of every
 *            level) replaces the keyframe, whose twist and id become the frame's.
 *   SKIP     the input is not read; keyframe, its pose and the frame counter stay; the world pose is kept (identity if the sequence
 *            never started); is_keyframe = 0.
 * Outputs: dvo_batch_last_poses / _copy_poses_device keep their convention (exp(xi) = inv(P_obj) P_ref) with the KEYFRAME as the
 * reference; dvo_batch_last_status, _last_track_log and _gather_poses_rccl keep their meaning.  dvo_batch_world_poses and
 * _copy_world_poses_device return the world twists / poses and keyframe flags (DVO_ERR_NOT_READY before the first push; a sensor-depth
 * batch without keyframe tracking still gets DVO_ERR_BAD_ARGUMENT).  dvo_batch_keyframe_get returns gray and depth of any level,
 * xi, id and n_keyframes (valid_updates = 0); sigma and age are not stored: non-NULL -> DVO_ERR_BAD_ARGUMENT; a sequence that never
 * started -> DVO_ERR_NOT_READY.  Start pose (dvo_batch_set_pose_guess_mode) follows the mono convention: GIVEN rows are WORLD
 * twists g and the tracker starts from se3_concatenate(-keyframe twist, g); CONSTANT_VELOCITY extrapolates the world twists;
 * dvo_batch_last_start_poses reports the keyframe-relative start.
 * Every push runs the per-sequence path (as after dvo_batch_set_actions).  A batch that never calls this runs exactly the launches it
 * always ran.  Errors, returned before anything changes: a NULL handle or a mono batch -> DVO_ERR_BAD_ARGUMENT; a call after the first
 * push, or (enable != 0) while a prefetched frame waits -> DVO_ERR_NOT_READY.  While keyframe tracking is on, dvo_batch_prefetch_* ->
 * DVO_ERR_NOT_READY, and a push whose weight storage differs from the keyframes' (float maps after raw frames or the reverse) ->
 * DVO_ERR_BAD_ARGUMENT. */
int dvo_batch_set_keyframe_tracking(dvo_batch* b, int enable);   /* sensor-depth batches; before the first push */
/* ---- keyframe depth fusion of a sensor-depth batch with keyframe tracking ---------------------------------------
 * A keyframe's depth map is the single measurement it was promoted with; every frame tracked against it measures the same surface
 * again.  dvo_batch_set_keyframe_fusion makes every later push fold the tracked frame's depth into the keyframe's map as a running
 * mean, after the push's tracking and keyframe decision (two kernels: k_kf_fuse_prep, one thread per sequence, and k_kf_fuse; no kernel of the tracker changes, and the push that
 * measured a depth never sees it: the fused map is the reference of the NEXT push).  A batch that never calls it runs exactly the
 * launches it always ran.
 * Contract: float32, IEEE, no contraction beyond the fmaf()s named.  T = levels - 1 (the top level, w x h), k = the sequence's
 * level-T intrinsics (with dvo_batch_set_intrinsics: its row of the per-sequence table), xi = the push's relative twist,
 * F = the float pose of exp(xi) (the T_rel of dvo_batch_last_poses: keyframe-camera points into the tracked frame), Bk = the float
 * pose of exp(-xi) (bit for bit dvo_op_se3_exp(-xi): the double-precision chain, rounded once).  Per sequence, after the keyframe
 * decision and the promotions of the push:
 *   STARTED, or TRACKED with the keyframe rule fired: the depth was just replaced; its count plane becomes 0, its record zeros.
 *   SKIPPED / BAD_ACTION: nothing of it is read or written; record zeros.
 *   TRACKED, rule not fired, all six components of xi finite (otherwise nothing is fused, record zeros): for every top-level (x, y)
 *    1. d = kf_depth[T][y][x]; the pixel is a CANDIDATE iff d >= min_depth (false for NaN: holes are never filled).
 *    2. back_project(k, (float)x, (float)y, d), transform(F, ...) -> (Xf, Yf, Zf); Zf >= min_depth; project(k, ...) -> (u, v).
 *    3. 0 <= u < w - 1 and 0 <= v < h - 1 (false for NaN / inf); x0 = (int)u, y0 = (int)v, a = u - (float)x0, b = v - (float)y0.
 *    4. the taps z00, z10, z01, z11 of the TRACKED frame's top-level depth at (x0, y0) .. (x0 + 1, y0 + 1): all >= min_depth and
 *       < inf, and max4 - min4 <= max_diff (no blend across a depth edge).
 *    5. top = fmaf(a, z10 - z00, z00), bot = fmaf(a, z11 - z01, z01), zi = fmaf(b, bot - top, top).
 *    6. fabsf(zi - Zf) <= max_diff.
 *    7. back_project(k, u, v, zi), transform(Bk, ...): d_obs = its z; d_obs >= min_depth and < inf.
 *    8. c = count[y][x], r = 1.0f / (float)(c + 2) (the IEEE quotient), d_new = fmaf(d_obs - d, r, d), c_new = min(c + 1, max_count):
 *       the running mean of the keyframe's own sample and c fused ones; an exponential average once c has reached max_count.
 *    9. c_new -> count; d_new -> kf_depth[T][y][x] and every coarser level l whose point decimation picks the pixel (t = T - l:
 *       x and y multiples of 2^t, (x >> t) < w_l, (y >> t) < h_l), so dvo_batch_keyframe_get returns the fused depth at every level.
 *   A candidate failing at 2, 3, 4 or 7 is unchanged; one failing only at 6 counts in n_gated; one reaching 9 counts in n_fused.  The
 *   counters are integer sums: order-free, deterministic.  Gray, sigma and the weight maps are not touched.
 * dvo_batch_set_keyframe_fusion: between any two pushes while keyframe tracking is on; from the next push on; cfg NULL or mode
 * DVO_KF_FUSION_OFF stops fusing and leaves the maps as they are.  Turning it on (from off) allocates the uint8 count plane
 * [n_seq][h][w] on first use and zeroes it.  dvo_batch_last_keyframe_fusion: the records [n_seq] of the last push (host,
 * synchronises; struct_size is set to sizeof(dvo_kf_fusion_record)); dvo_batch_keyframe_fusion_counts: the count plane of one
 * sequence (host, synchronises).
 * Errors, returned before anything is enqueued or changed: a NULL handle (or NULL output) or a mono batch -> DVO_ERR_BAD_ARGUMENT; a
 * sensor-depth batch without keyframe tracking -> DVO_ERR_NOT_READY; mode outside {0, 1}, max_diff not finite or <= 0, max_count
 * outside [1, 255], seq out of range -> DVO_ERR_BAD_ARGUMENT; a reader before a push that ran with fusion on -> DVO_ERR_NOT_READY.
 * All three fields of a non-NULL cfg are checked whatever the mode: to turn fusion off pass NULL, or a valid configuration (one from
 * dvo_kf_fusion_config_default) with mode = DVO_KF_FUSION_OFF; a zeroed struct is refused for its max_diff and max_count.
 * With keyframe tracking on, dvo_batch_frame_get returns the frame of the last push (the tracked frame this fusion read; on the
 * first push the keyframe itself). */
#define DVO_KF_FUSION_OFF 0
#define DVO_KF_FUSION_ON  1
typedef struct dvo_kf_fusion_config { int mode; float max_diff; int max_count; } dvo_kf_fusion_config;
void dvo_kf_fusion_config_default(dvo_kf_fusion_config* cfg);   /* DVO_KF_FUSION_ON, max_diff = 0.05, max_count = 16 */
int dvo_batch_set_keyframe_fusion(dvo_batch* b, const dvo_kf_fusion_config* cfg);   /* from the next push on; NULL cfg = OFF */
typedef struct dvo_kf_fusion_record { int struct_size, n_candidates, n_fused, n_gated; } dvo_kf_fusion_record;
int dvo_batch_last_keyframe_fusion(dvo_batch* b, dvo_kf_fusion_record* rec /*[n_seq]*/);   /* host, synchronises */
int dvo_batch_keyframe_fusion_counts(dvo_batch* b, int seq, uint8_t* counts /*[h_top][w_top]*/);
/* ---- keyframe carry: fused depth and counts survive a promotion --------------------------------------------------
 * Without it a promotion copies the tracked frame's single measurement over the fused map and the counts restart at 0.
 * dvo_batch_set_keyframe_carry makes every later promotion blend the old keyframe's fused depth, warped into the frame that becomes
 * the keyframe, into that frame's depth before it is copied, and carry the counts along (three kernels: k_kf_carry_prep, k_kf_carry,
 * k_kf_carry_commit; no existing kernel changes).  A batch that never calls it runs exactly the launches it always ran.
 * Contract: float32, IEEE, no contraction beyond the fmaf()s named; T, k, xi, F = the float pose of exp(xi) and Bk = the float pose
 * of exp(-xi) (bit for bit dvo_op_se3_exp(-xi)) as for the fusion above.  The carry runs on a push that TRACKED the sequence with the
 * keyframe rule fired and all six components of xi finite, after the keyframe decision and BEFORE the tracked frame is copied over
 * the keyframe.  For every top-level pixel (x, y) of the TRACKED frame (the keyframe-to-be):
 *    1. d = frame_depth[T][y][x]; the pixel is a CANDIDATE iff d >= min_depth and d < inf (false for NaN: holes are never filled).
 *    2. back_project(k, (float)x, (float)y, d), transform(Bk, ...) -> (Xk, Yk, Zk); Zk >= min_depth; project(k, ...) -> (u, v).
 *    3. 0 <= u < w - 1 and 0 <= v < h - 1 (false for NaN / inf); x0 = (int)u, y0 = (int)v, a = u - (float)x0, b = v - (float)y0.
 *    4. the taps z00, z10, z01, z11 of the OLD keyframe's top-level depth at (x0, y0) .. (x0 + 1, y0 + 1): all >= min_depth and
 *       < inf, and max4 - min4 <= max_diff.
 *    5. top = fmaf(a, z10 - z00, z00), bot = fmaf(a, z11 - z01, z01), zi = fmaf(b, bot - top, top).
 *    6. fabsf(zi - Zk) <= max_diff (the carry's own max_diff).
 *    7. back_project(k, u, v, zi), transform(F, ...): d_prior = its z; d_prior >= min_depth and < inf.
 *    8. c_prior = the minimum of the four taps' counts: the old map stands for c_prior + 1 samples, the pixel's own measurement for
 *       one.  r = (float)(c_prior + 1) * (1.0f / (float)(c_prior + 2)) (the IEEE quotient, then one rounded product),
 *       d_new = fmaf(d_prior - d, r, d); d_new >= min_depth and < inf.
 *    9. c_new = min(c_prior + 1, max_count) with the fusion's max_count; d_new -> the frame's depth at level T and at every coarser
 *       level whose point decimation picks the pixel, as the fusion's step 9; the copy then makes it the keyframe.
 *   A pixel that fails anywhere keeps d and gets count 0; a candidate failing only at 6 counts in n_gated, one reaching 9 in
 *   n_carried.  The counters are integer sums: order-free, deterministic.  Gray, sigma and the weight maps are not touched.
 *   STARTED sequences, and TRACKED ones whose rule fired with a non-finite xi, clear as without the carry; SKIPPED / BAD_ACTION: nothing
 *   is read or written; TRACKED without the rule firing: the fusion above.  Records of sequences that did not carry are zeros.
 * The carried depth is written into the tracked frame's own pyramid: after a carrying push dvo_batch_frame_get returns the carried
 * depth for the promoted sequences (it is what became the keyframe) and the untouched frame for the others.
 * dvo_batch_set_keyframe_carry: between any two pushes while keyframe tracking and fusion are on; from the next push on; cfg NULL or
 * mode DVO_KF_CARRY_OFF stops carrying and leaves maps and counts as they are; turning fusion off turns the carry off.  The first
 * use allocates a uint8 staging plane [n_seq][h][w].  dvo_batch_last_keyframe_carry: the records [n_seq] of the last push (host,
 * synchronises; struct_size is set to sizeof(dvo_kf_carry_record)).
 * Errors, returned before anything is enqueued or changed: a NULL handle (or NULL output) or a mono batch -> DVO_ERR_BAD_ARGUMENT;
 * no keyframe tracking, or fusion not on -> DVO_ERR_NOT_READY; struct_size != sizeof(dvo_kf_carry_config), mode outside {0, 1},
 * max_diff not finite or <= 0 -> DVO_ERR_BAD_ARGUMENT; the reader before a push that ran with carry on -> DVO_ERR_NOT_READY. */
#define DVO_KF_CARRY_OFF 0
#define DVO_KF_CARRY_ON  1
typedef struct dvo_kf_carry_config { int struct_size; int mode; float max_diff; } dvo_kf_carry_config;
void dvo_kf_carry_config_default(dvo_kf_carry_config* cfg);   /* struct_size, DVO_KF_CARRY_ON, max_diff = 0.05 */
int dvo_batch_set_keyframe_carry(dvo_batch* b, const dvo_kf_carry_config* cfg);   /* from the next push on; NULL cfg = OFF */
typedef struct dvo_kf_carry_record { int struct_size, n_candidates, n_carried, n_gated; } dvo_kf_carry_record;
int dvo_batch_last_keyframe_carry(dvo_batch* b, dvo_kf_carry_record* rec /*[n_seq]*/);   /* host, synchronises */
/* ---- keyframe maps as compacted world-frame point clouds, on the device ------------------------------------------
 * dvo_batch_export_points writes the semi-dense point set of every sequence's current keyframe into the caller's device buffers:
 * a mono batch, or a sensor-depth batch with keyframe tracking.  Asynchronous, in stream order on the handle's stream; it reads the
 * state the last push / call left and changes nothing in the handle's maps.  A batch that never calls it runs exactly the launches
 * it always ran.
 * Candidates: pixel (x, y) of level `level` (w_l x h_l) of a selected sequence with x % stride == 0 && y % stride == 0, d = the
 * keyframe depth of that level (what dvo_batch_keyframe_get returns) with d >= min_depth && d <= max_depth (false for NaN / inf),
 * and, where set: sigma[level][y][x] <= max_sigma (mono; +inf = no gate: the map is not read), age[y][x] >= min_age (mono, top level;
 * 0 = no gate), count[y][x] >= min_count (sensor depth after a push that ran with keyframe fusion, top level; 0 = no gate).
 * Selected: DVO_POINTS_ALL every sequence that has started; DVO_POINTS_NEW those of them whose last push / call made a keyframe
 * (is_keyframe = 1 of dvo_batch_world_poses).  The others contribute no points.
 * Order: sequences in index order, within a sequence raster order of the level.  offsets[s] = index of sequence s's first point,
 * offsets[n_seq] = the total; for point i of sequence s: src[i] = y * w_l + x, xyzg[i] = (Xw, Yw, Zw, gray[level][y][x]),
 * sigma[i] = sigma[level][y][x] (mono only).
 * Arithmetic: float32, IEEE, no contraction beyond the fmaf()s named (as above): back_project(k_l, (float)x, (float)y, d) with the
 * sequence's own level intrinsics (its row of the per-sequence table where the batch has one), then transform(Wk, ...), Wk = the
 * float pose of exp(-ref_xi), bit for bit dvo_op_se3_exp(-ref_xi), ref_xi = the keyframe's world twist (xi of
 * dvo_batch_keyframe_get): exp(ref_xi) takes world points into the keyframe camera (frame_xi = concatenate(ref_xi, rel_xi) and
 * exp(rel_xi) takes keyframe-camera points into the tracked frame), so exp(-ref_xi) takes keyframe-camera points into the world.  The
 * first keyframe sits at the identity.  A keyframe twist that is not finite gives coordinates that are not finite.
 * Capacity: the offsets are always the full ones; a point whose index is >= capacity is not written and nothing at or past capacity
 * is touched; capacity = 0 with NULL xyzg / src / sigma is the counting call.  dvo_batch_last_points copies the offsets of the last
 * export to the host (synchronises), so the caller can compare offsets[n_seq] with its capacity.
 * Errors, returned before anything is enqueued: a NULL handle, cfg or offsets_dev, or a plain sensor-depth batch ->
 * DVO_ERR_BAD_ARGUMENT; before the first push / call -> DVO_ERR_NOT_READY; struct_size != sizeof(dvo_points_config), select outside
 * {0, 1}, level outside [0, levels) and not -1, stride < 1, min_depth not finite, max_depth NaN or < min_depth, max_sigma NaN, a gate set where
 * it does not apply (max_sigma != +inf or sigma_dev on a sensor-depth batch; min_age != 0 off a mono batch's top level, or negative
 * or not finite; min_count != 0 off the top level of a sensor-depth batch that has fused, or outside [0, 255]), capacity > 0 with a
 * NULL xyzg_dev or one not 16-byte aligned, capacity > 2^31 - 1, n_seq * w_l * h_l > 2^31 - 1, w_l * h_l > 2^24 ->
 * DVO_ERR_BAD_ARGUMENT; per-sequence intrinsics changed (dvo_batch_set_intrinsics) since the last push -> DVO_ERR_NOT_READY (the
 * keyframes belong to the cameras of that push); dvo_batch_last_points before an export -> DVO_ERR_NOT_READY. */
#define DVO_POINTS_ALL 0   /* every started sequence's current keyframe */
#define DVO_POINTS_NEW 1   /* only sequences whose last push / call made a keyframe (is_keyframe = 1) */
typedef struct dvo_points_config {
    int   struct_size;     /* sizeof(dvo_points_config) */
    int   select;          /* DVO_POINTS_ALL / _NEW */
    int   level;           /* pyramid level of the keyframe maps, 0 .. levels-1; -1 (the default) = levels-1, the top level */
    int   stride;          /* >= 1: pixel (x, y) is a candidate iff x % stride == 0 && y % stride == 0 */
    float min_depth, max_depth;   /* candidate iff d >= min_depth && d <= max_depth (false for NaN / inf); min_depth < 0 (the
                                     default, -1) = the handle's dvo_config::min_depth */
    float max_sigma;       /* mono: sigma[level] <= max_sigma; +inf = no gate.  Sensor depth: must be +inf */
    float min_age;         /* mono, top level only: age >= min_age; 0 = no gate.  Elsewhere must be 0 */
    int   min_count;       /* sensor depth with keyframe fusion on, top level only: count >= min_count; 0 = no gate.  Elsewhere must be 0 */
} dvo_points_config;
void dvo_points_config_default(dvo_points_config* cfg);   /* ALL, top level, stride 1, the handle's min_depth, max_depth +inf, no other gate */
int dvo_batch_export_points(dvo_batch* b, const dvo_points_config* cfg, uint32_t capacity,
                            float* xyzg_dev /*[capacity][4]*/, uint32_t* src_dev /*[capacity] or NULL*/,
                            float* sigma_dev /*[capacity] or NULL; mono only*/, uint32_t* offsets_dev /*[n_seq + 1]*/);
int dvo_batch_last_points(dvo_batch* b, uint32_t* offsets /*[n_seq + 1], host; synchronises*/);
/* ---- per-sequence tracking quality (both batch kinds) ---------------------------------------------------------------------------
 * dvo_batch_set_track_quality(b, 1) makes every later push / call keep, per sequence, the sums of the LAST Gauss-Newton iteration of
 * the finest level (levels - 1: the solve that produced the returned pose); enable = 0 stops keeping them.  Poses, status, world
 * poses, track logs and every schedule are unchanged; a batch that never enables it runs exactly the launches it always ran.
 * dvo_batch_last_track_quality (host, synchronises) and dvo_batch_copy_track_quality_device (device, asynchronous, in stream order on
 * the handle's stream) write one record per sequence [n_seq] describing the LAST push / call; a later read of the same push gives the
 * same records (pushes in between are what changes them).  Per record:
 *   status       that push's DVO_SEQ_TRACKED / SKIPPED / STARTED / BAD_ACTION, as dvo_batch_last_status / _mono_last_status.
 *   n_iter       the track log's n_iter (0 beyond the batch's levels).
 *   H, g, sum_r2, n_valid   bit for bit the sums that iteration's 6x6 solve used: H = upper triangle of sum J^T J row by row (index
 *                of (i, j), i <= j: i*6 - i*(i-1)/2 + j - i), g = sum J^T (w r).  They are evaluated at that iteration's INPUT pose
 *                (the pose before its update), not at the returned pose, as Gauss-Newton forms them.
 *   residual     sum_r2 / n_valid in float (optimize.cpp:98), -1 when n_valid == 0; update_norm = |xi_update| of that iteration.
 *                Both are the track log's entries bit for bit.
 *   eigenvalues  of H (symmetric), ascending, by Jacobi rotations in double; NaN when a sum (H, g or sum_r2) is not finite.
 *   covariance   upper triangle (as H) of s2 * H^-1, s2 = sum_r2 / (n_valid - 6), in the coordinates of the twist the tracker updates
 *                (xi <- log(exp(xi) exp(upd)), tracker.cpp:46): relative to the reference (the keyframe in keyframe mode and mono),
 *                as dvo_batch_last_poses and the mono tracker's relative twist.  NaN when n_valid <= 6, when RANK_DEFICIENT is set,
 *                when a sum is not finite or when an eigenvalue is not positive.  It is the least-squares covariance of the problem as
 *                the reference forms it: a consistent relative confidence, not a calibrated metric covariance.
 *   flags        DVO_QUALITY_*:
 *     CONVERGED        the finest level stopped on min_update or min_residual (tracker.cpp:68-73); fixed_iterations = 0 only.
 *     CAPPED           the finest level ran max_iterations without either test firing; fixed_iterations = 0 only.
 *     NO_VALID         n_valid == 0 in that iteration (residual -1, optimize.cpp:92-93).
 *     NOT_FINITE       that iteration's update had a component that is not finite: the pose kept its value (tracker.cpp:46-51).
 *     RANK_DEFICIENT   the 6x6 solve judged H singular and took the pseudo-inverse: the largest diagonal entry is > 0 and an LDL^T
 *                      pivot is <= 1e-12 times it.  An all-zero (or all non-finite) diagonal gives a zero update without the
 *                      pseudo-inverse and does not set it.
 * A sequence that did not track at that push (SKIPPED, STARTED, BAD_ACTION) gets the empty record: n_valid = 0, n_iter all 0,
 * flags = 0, residual -1, update_norm 0, sum_r2 / H / g zero, eigenvalues and covariance NaN -- never an earlier push's data.
 * struct_size = sizeof(dvo_track_quality) of the library (the struct may grow at its end).
 * Errors: a NULL handle or a NULL output -> DVO_ERR_BAD_ARGUMENT; a read before a push / call that ran with quality enabled (or after
 * one that ran with it disabled) -> DVO_ERR_NOT_READY.  dvo_vo handles have no quality record (dvo_vo_last_track_log). */
#define DVO_QUALITY_CONVERGED       1
#define DVO_QUALITY_CAPPED          2
#define DVO_QUALITY_NO_VALID        4
#define DVO_QUALITY_NOT_FINITE      8
#define DVO_QUALITY_RANK_DEFICIENT 16
typedef struct dvo_track_quality {
    int    struct_size;
    int    status;
    int    flags;
    int    n_valid;
    int    n_iter[DVO_MAX_LEVELS];
    float  residual;
    float  update_norm;
    double sum_r2;
    double H[21];
    double g[6];
    double eigenvalues[6];
    double covariance[21];
} dvo_track_quality;
int dvo_batch_set_track_quality(dvo_batch* b, int enable);                      /* both kinds; from the next push / call on */
int dvo_batch_last_track_quality(dvo_batch* b, dvo_track_quality* out);         /* [n_seq], host, synchronises */
int dvo_batch_copy_track_quality_device(dvo_batch* b, dvo_track_quality* dst);  /* [n_seq], device, asynchronous on the handle's stream */
/* ---- robust residual weights (both batch kinds) ---------------------------------------------------------------------------------
 * By default every contributing pixel enters the normal equations with full weight.  dvo_batch_set_robust_weights makes every later
 * push / call run iteratively reweighted least squares: per sequence and Gauss-Newton iteration a squared scale s2 (float) and per
 * contributing pixel a weight rho of its residual r (J, r, rw as the plain estimator forms them; gates, samplers, n_valid and the
 * mask at a given pose are unchanged), all float32:
 *   DVO_ROBUST_HUBER       c = param * sqrtf(s2);                  rho = fabsf(r) <= c ? 1 : c / fabsf(r)        (param = k > 0)
 *   DVO_ROBUST_STUDENT_T   A = (param + 1) * s2, B = param * s2;   rho = A / fmaf(r, r, B)                       (param = nu > 0)
 *   "plain"                rho = 1 exactly: the unweighted term bit for bit.
 * The sums keep their slots and order: Jr[p] = rho * J[p]; H[p][q] += Jr[p] * J[q]; g[p] += Jr[p] * rw; sum_r2 += (rho * r) * r.
 * residual = (float)sum_r2 / (float)n_valid is therefore the WEIGHTED mean square: that value is what the track log, the min_residual
 * stop test and the quality record (dvo_batch_last_track_quality) see while weights are on.
 * The scale, by scale_mode:
 *   DVO_ROBUST_SCALE_ADAPTIVE   s2 = max(residual_prev, scale_floor * scale_floor), residual_prev = the sequence's logged residual of
 *                               its previous iteration in this push (the same level, or the coarser level's last iteration at a
 *                               level's first): one fixed-point step of the IRLS scale per iteration -- a weighted RMS, not a MAD.
 *                               Plain on the first iteration of the coarsest level and whenever residual_prev is not > 0 (the -1 of an
 *                               iteration without pixels).
 *   DVO_ROBUST_SCALE_GIVEN      s2 = s[seq] * s[seq], the rows of dvo_batch_set_robust_scales ([n_seq]; host rows are copied before
 *                               the call returns, device rows are read in stream order by every later push; NULL clears).  A sequence
 *                               whose s is not finite and > 0 (or whose s * s is not), and every sequence while no rows are set, is plain.
 * Takes effect from the next push / call; cfg == NULL or kind == DVO_ROBUST_NONE turns the weights off again, and the batch then runs
 * exactly the launches it ran before.  A batch that never calls this runs exactly the launches it always ran.  While on, every level
 * runs launch pairs (k_track_gn_rw + k_gn_solve_rw) whatever track_fused_tiles, gn_use_lds_patch and track_single_launch say.
 * dvo_batch_last_robust_scales: s2[n_seq] (host, synchronises) -- the s2 of the finest level's last iteration of the last push per
 * sequence, +inf where that iteration was plain, 0 for a sequence that did not track at that push.
 * Errors, returned before anything is enqueued: a NULL handle, a kind or mode outside the sets, param or scale_floor not finite
 * and > 0 (whatever the mode), struct_size != sizeof(dvo_robust_config), rows outside the GIVEN mode -> DVO_ERR_BAD_ARGUMENT;
 * dvo_batch_last_robust_scales before a push that ran with weights on -> DVO_ERR_NOT_READY.  dvo_vo handles have no robust weights. */
#define DVO_ROBUST_NONE      0
#define DVO_ROBUST_HUBER     1
#define DVO_ROBUST_STUDENT_T 2
#define DVO_ROBUST_SCALE_ADAPTIVE 0
#define DVO_ROBUST_SCALE_GIVEN    1
typedef struct dvo_robust_config {
    int   struct_size;   /* sizeof(dvo_robust_config) */
    int   kind;          /* DVO_ROBUST_* */
    int   scale_mode;    /* DVO_ROBUST_SCALE_* */
    float param;         /* Huber k / Student-t nu, > 0 */
    float scale_floor;   /* > 0; adaptive: s2 never falls below scale_floor^2 */
} dvo_robust_config;
int dvo_batch_set_robust_weights(dvo_batch* b, const dvo_robust_config* cfg);   /* both kinds; from the next push / call on */
int dvo_batch_set_robust_scales(dvo_batch* b, const float* s, int s_on_device); /* [n_seq], GIVEN mode; NULL clears */
int dvo_batch_last_robust_scales(dvo_batch* b, float* s2);                      /* [n_seq], host, synchronises */
/* ---- the median (MAD) robust scale (both batch kinds) ----------------------------------------------------------------------------
 * dvo_batch_set_robust_median turns the robust weights on with a third scale rule, DVO_ROBUST_SCALE_MEDIAN: per sequence and
 * Gauss-Newton iteration s2 comes from the median of |r| over the contributing pixels of the PREVIOUS evaluation, found from 256 exact
 * bin counts.  The residuals are treated as centred (no subtraction of a median of r).  A 50 %-breakdown scale, where the adaptive
 * rule is a weighted RMS.  kind is DVO_ROBUST_HUBER or DVO_ROBUST_STUDENT_T, scale_mode must be DVO_ROBUST_SCALE_MEDIAN, param and
 * scale_floor are validated as dvo_batch_set_robust_weights validates them.  cfg == NULL, or dvo_batch_set_robust_weights with
 * DVO_ROBUST_NONE / NULL, turns it off.  The contract, float32 and integer, IEEE, no contraction:
 *   Bin.       r = the unweighted residual robust_rho sees.  K0 = (127 - 16) << 4 = 1776;
 *              bin = clamp((int)(__float_as_uint(fabsf(r)) >> 19) - 1776, 0, 255): 16 bins per octave over [2^-16, 1), everything
 *              smaller in bin 0, everything larger (and NaN) in bin 255.
 *   Counts.    Every contributing pixel is counted: sum counts = n_valid exactly.  A rejected pixel (rho forced to 1) is not counted.
 *   Histogram. counts[256] per sequence are exact integer sums over all tiles of the launch, main loop and deferred border loop
 *              alike: independent of tile shape, launch plan, track_streams and summation order.
 *   Median.    n = sum counts.  n == 0: the next entry is plain.  Otherwise m = the smallest bin with cum(m) >= (n + 1) / 2 (integer
 *              division); med = __uint_as_float(((m + 1776) << 19) | (1 << 18)), the bin's midpoint; s = 1.4826f * med;
 *              s2 = max(s * s, floor2), floor2 = scale_floor * scale_floor; the next launch's weights are those of (kind, param, s2).
 *   Lag and priming.  Iteration i uses the entry written by the solve of iteration i - 1 (the same level, or the coarser level's last
 *              iteration), as the adaptive rule does.  The first iteration of the coarsest level uses the entry of a priming pair: one
 *              tile launch plus solve on the coarsest level at the start pose, which writes the entry and the priming slot of the log
 *              and nothing else: no pose, no track log, no quality record.
 *   Weights and sums.  Everything downstream of s2 (rho, the weighted sums, the weighted residual) is dvo_batch_set_robust_weights'.
 * While on, every level runs launch pairs (k_track_gn_md + k_gn_solve_md).  dvo_batch_last_robust_scales reports the s2 the finest
 * level's last solve used, as in the other modes.  dvo_batch_last_robust_log (host, synchronises): per level and iteration, indexed
 * like dvo_track_log, the s2 the iteration USED and the median bin m and count n of that iteration's pixels, which produced the NEXT
 * entry (m = -1 where n = 0), and the priming pair's (m, n); empty (n_iter all 0) for a sequence that did not track.
 * dvo_batch_last_robust_histogram (host, synchronises): counts[256] of the finest level's last iteration, zeros for a sequence that
 * did not track.
 * Errors, returned before anything is enqueued: a NULL handle, a config that fails dvo_batch_set_robust_weights' checks, a kind of
 * DVO_ROBUST_NONE, a scale_mode other than DVO_ROBUST_SCALE_MEDIAN, affine brightness or the geometric term on ->
 * DVO_ERR_BAD_ARGUMENT.  While it is on, dvo_batch_set_affine_brightness, dvo_batch_set_geometric and
 * dvo_batch_set_geometric_affine refuse, and so does dvo_batch_set_robust_scales (there are no given rows).  The readers before a push that ran in this mode -> DVO_ERR_NOT_READY. */
#define DVO_ROBUST_SCALE_MEDIAN   2
typedef struct dvo_robust_log {
    int   struct_size;    /* sizeof(dvo_robust_log), set by the caller */
    int   levels;
    int   n_iter[DVO_MAX_LEVELS];
    float s2[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];          /* the s2 the iteration used (+inf: plain) */
    int   median_bin[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];  /* m of the iteration's own pixels: the next entry's (-1: n = 0) */
    int   count[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];       /* n = sum counts = n_valid */
    int   prime_bin, prime_count;                          /* the priming pair's (m, n) */
} dvo_robust_log;
int dvo_batch_set_robust_median(dvo_batch* b, const dvo_robust_config* cfg);      /* both kinds; from the next push / call on */
int dvo_batch_last_robust_log(dvo_batch* b, int seq, dvo_robust_log* log);        /* host, synchronises */
int dvo_batch_last_robust_histogram(dvo_batch* b, int seq, uint32_t counts[256]); /* host, synchronises */
/* ---- affine brightness compensation: gain and offset (both batch kinds) ---------------------------------------------------------
 * By default every residual is r = I2 - I1: brightness constancy.  dvo_batch_set_affine_brightness makes every later push / call
 * track under the photometric model I2(warp(x)) ~ a * I1(x) + b with one (a, b) per sequence (auto-exposure, auto-gain), I1 and I2
 * in the roles they have in the plain residual: I1 the tracked frame's own pixel, I2 the reference sampled at the warped position.
 * All arithmetic is float32 and IEEE, with no contraction beyond the fmaf()s named.
 * Per contributing pixel (J, the gates, the samplers, n_valid and the mask at a given pose are the plain estimator's):
 *   c = fmaf(a, I1, b);  r = I2 - c;  rw = r * wgt.  With (a, b) = (1, 0) c is I1 exactly: every term is the plain term bit for bit.
 *   The 29 sums keep their slots, their fmaf shape and their reduction, with this r; with robust weights on too
 *   (dvo_batch_set_robust_weights), rho is taken of the compensated r and the sums are the weighted ones.
 * Brightness moments of the same pixels (rho = 1 without robust weights), p = rho * I1 rounded once:
 *   M0 += rho;  M1 += p;  M2 = fmaf(rho, I2, M2);  M11 = fmaf(p, I1, M11);  M12 = fmaf(p, I2, M12);  a rejected pixel adds exact zeros.
 *   They are reduced in a fixed order of their own (wave, the four waves in wave order, the tiles in double), the same under every
 *   schedule.  Without robust weights M0 is not kept: N below is n_valid.
 * The next entry, in double from the double totals, N = M0 (robust weights on) or n_valid:
 *   det = N * M11 - M1 * M1;  a' = (N * M12 - M1 * M2) / det;  b' = (M2 - a' * M1) / N
 *   The entry becomes ((float)a', (float)b') only when n_valid >= min_pixels, det > min_contrast * N * M11 (a scale-free flat-image
 *   guard), both values are finite and gain_min <= a' <= gain_max; otherwise it keeps its value.
 * The estimate alternates: every Gauss-Newton iteration applies the (a, b) of its entry and accumulates the moments, and the solve
 * writes the closed form of those moments as the next launch's entry.  J does not depend on (a, b): the 6x6 solve, the track log and
 * the quality record keep their shape.  It is not a joint 8-parameter Gauss-Newton, and there is no per-pixel model (vignetting,
 * response curve).  The mode:
 *   DVO_AFFINE_ESTIMATE   every tracking call starts each tracked sequence at (1, 0).  A priming pair runs first, on the coarsest level
 *                         at the start pose: it accumulates the moments with rho = 1 and writes the entry -- nothing else (no pose,
 *                         log, iteration count, active list or quality record).  After it every iteration uses the entry the launch
 *                         before it wrote; the entry carries across levels.  (With the adaptive robust scale the first iteration of the
 *                         coarsest level is still unweighted: the priming pair leaves the weight table alone.)
 *   DVO_AFFINE_GIVEN      (a, b) = the rows of dvo_batch_set_affine_rows ([n_seq][2]; host rows are copied before the call returns,
 *                         device rows are read in stream order by every later push; NULL clears), fixed for the whole call, no priming
 *                         pair.  A row that is not finite or has a <= 0, and every sequence while no rows are set, is (1, 0).
 * Takes effect from the next push / call; cfg == NULL or mode == DVO_AFFINE_OFF turns it off again, and the batch then runs exactly
 * the launches it ran before.  A batch that never calls this runs exactly the launches it always ran.  While on, every level runs
 * launch pairs (k_track_gn_ab + k_gn_solve_ab) whatever track_fused_tiles, gn_use_lds_patch and track_single_launch say.
 * A mono batch applies the compensation to the tracking only: the depth filter's SSD search still assumes brightness constancy.
 * dvo_batch_last_affine: ab[n_seq][2] (host, synchronises) -- the entry the finest level's last iteration of the last push used,
 * (0, 0) for a sequence that did not track at that push.  dvo_batch_last_affine_log: the entry every logged iteration USED, indexed
 * like dvo_track_log (so a replay has the device's own bits), and the entry the priming pair wrote ((0, 0) in GIVEN mode); empty
 * (n_iter all 0) for a sequence that did not track.
 * Errors, returned before anything is enqueued: a NULL handle, a mode outside the set, struct_size != sizeof, min_pixels < 2,
 * min_contrast outside [0, 1), a gain range without 0 < gain_min <= gain_max < inf, rows outside the GIVEN mode ->
 * DVO_ERR_BAD_ARGUMENT; a read before a push that ran with the feature on -> DVO_ERR_NOT_READY.  dvo_vo handles have no compensation. */
#define DVO_AFFINE_OFF      0
#define DVO_AFFINE_ESTIMATE 1
#define DVO_AFFINE_GIVEN    2
typedef struct dvo_affine_config {
    int   struct_size;    /* sizeof(dvo_affine_config) */
    int   mode;           /* DVO_AFFINE_* */
    int   min_pixels;     /* >= 2: fewer contributing pixels keep the entry */
    float min_contrast;   /* [0, 1): det <= min_contrast * N * M11 keeps the entry */
    float gain_min;       /* 0 < gain_min <= gain_max: an a' outside keeps the entry */
    float gain_max;
} dvo_affine_config;
typedef struct dvo_affine_log {
    int   struct_size;    /* sizeof(dvo_affine_log), set by the caller */
    int   levels;
    int   n_iter[DVO_MAX_LEVELS];
    float a[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    float b[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    float prime_a, prime_b;
} dvo_affine_log;
int dvo_batch_set_affine_brightness(dvo_batch* b, const dvo_affine_config* cfg);  /* both kinds; from the next push / call on */
int dvo_batch_set_affine_rows(dvo_batch* b, const float* ab, int ab_on_device);   /* [n_seq][2], GIVEN mode; NULL clears */
int dvo_batch_last_affine(dvo_batch* b, float* ab);                               /* [n_seq][2], host, synchronises */
int dvo_batch_last_affine_log(dvo_batch* b, int seq, dvo_affine_log* log);        /* host, synchronises */
/* ---- geometric (depth) term: sensor-depth batches only ---------------------------------------------------------------------------
 * By default a sensor-depth batch uses a frame's depth map only as the lever arm of the photometric residual, and the depth at pixel
 * x is the REFERENCE's (the reference's own approximation, GnArgs::ref_depth).  dvo_batch_set_geometric makes every later push add a
 * depth-error row per pixel: dense RGB-D alignment.  All arithmetic is float32 and IEEE, with no contraction beyond the fmaf()s named.
 * While on, pixel x of the TRACKED frame uses that frame's own values at x: d = the tracked frame's depth, wgt = the weight of the
 * tracked frame's own sigma (or its constant for raw frames), I1 = the tracked frame's gray.  (u, v) and Zw are the outputs of
 * warp's operations (back_project, transform, project): Zw is the transformed point's z.  I2, gx, gy are the samplers on the
 * reference gray.  The photometric row is the plain estimator's on these inputs, bit for bit: the gates, the samplers and the
 * Jacobian are unchanged, slots 0..28 keep their meaning, and n_valid, the residual and the stop tests stay photometric.
 * A contributing pixel also gets a geometric row when 1 <= u < w-2 and 1 <= v < h-2, all 12 gray taps of its footprint are valid
 * (the fast sampler decides it), all 12 taps D** of the REFERENCE depth at the same footprint are finite and >= min_depth, and
 * fabsf(rz) <= max_diff, where with hx = u - (int)u, vy = v - (int)v and blend4 the bilinear blend of the gray sampler:
 *   Zs  = blend4(D00, D01, D10, D11, hx, vy)
 *   gzx = blend4 of the four unhalved horizontal differences, gzy = blend4 of the four unhalved vertical differences (the gray
 *         sampler's three calls, applied to the depth taps)
 *   rz  = Zs - Zw
 *   Jp[6] = the photometric Jacobian formula with (gx, gy) := (gzx, gzy) (gn_jacobian_pre(k, x, y, d, iz, ., gzx, gzy, ., .))
 *   Jz = Jp except Jz[2] = Jp[2] - 1, Jz[3] = Jp[3] - Y, Jz[4] = Jp[4] + X, (X, Y) the back-projected point: the z-row of [I | -X^]
 *        under the unwarped-point convention and sign of the photometric J
 *   lam = weight * (iz * iz);  Jg[q] = lam * Jz[q];  rg = lam * rz;  rgw = rg * wgt      (iz = 1 / d: an inverse-depth-like error)
 * Sums, after the pixel's photometric add: slots 0..26 take (Jg, rgw) in the photometric fmaf shape (H[p][q] = fmaf(Jg[p], Jg[q], H),
 * g[p] = fmaf(Jg[p], rgw, g)); slots 27 and 28 are untouched; S29 = fmaf(rg, rg, S29) and S30 += 1 (n_geo).  A pixel without a
 * geometric row adds exact zeros: its operands are selected to zero first, so a NaN or inf tap never reaches a sum.  Pixels of the
 * border band and pixels with an INVALID gray tap (the generic sampler's) keep their photometric row and never get a geometric one.
 * S29 and S30 are reduced in a fixed order (wave, the four waves in wave order, the tiles in double), the same under every schedule.
 * weight = 0 is allowed: the 27 sums are then the plain estimator's on own-depth inputs, bit for bit.  The 6x6 solve, the track log
 * and the quality record keep their arithmetic: they see the combined H and g.
 * Takes effect from the next push; cfg == NULL or mode == DVO_GEOMETRIC_OFF turns it off again, and the batch then runs exactly the
 * launches it ran before.  A batch that never calls this runs exactly the launches it always ran.  While on, every level runs launch
 * pairs (k_track_gn_z + k_gn_solve_z) whatever track_fused_tiles, gn_use_lds_patch and track_single_launch say, and a big batch's
 * raw frames are not built in two halves.
 * dvo_batch_last_geometric: rec[n_seq] (host, synchronises) -- n_geo and mean_sq = S29 / n_geo (0 when n_geo is 0) of the finest
 * level's last iteration of the last push; zeros for a sequence that did not track at that push.  dvo_batch_last_geometric_log:
 * n_geo and (float)S29 of every logged iteration, indexed like dvo_track_log; empty (n_iter all 0) for a sequence that did not track.
 * Errors, returned before anything is enqueued: a NULL handle, struct_size != sizeof, a mode outside the set, a weight that is not
 * finite and >= 0, a max_diff that is not finite and > 0, a mono batch, robust weights or affine compensation on (in either order of
 * the two calls: dvo_batch_set_robust_weights / dvo_batch_set_affine_brightness refuse while this is on) -> DVO_ERR_BAD_ARGUMENT; a
 * read before a push that ran with the feature on -> DVO_ERR_NOT_READY.  dvo_vo handles have no geometric term. */
#define DVO_GEOMETRIC_OFF 0
#define DVO_GEOMETRIC_ON  1
typedef struct dvo_geometric_config {
    int   struct_size;    /* sizeof(dvo_geometric_config) */
    int   mode;           /* DVO_GEOMETRIC_* */
    float weight;         /* >= 0, finite */
    float max_diff;       /* > 0, finite, metres: |rz| above it has no geometric row */
} dvo_geometric_config;
typedef struct dvo_geometric_record {
    int   n_geo;          /* geometric rows of the finest level's last iteration */
    float mean_sq;        /* S29 / n_geo */
} dvo_geometric_record;
typedef struct dvo_geometric_log {
    int   struct_size;    /* sizeof(dvo_geometric_log), set by the caller */
    int   levels;
    int   n_iter[DVO_MAX_LEVELS];
    int   n_geo[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];
    float sum_sq[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];   /* (float)S29 */
} dvo_geometric_log;
void dvo_geometric_config_default(dvo_geometric_config* cfg);                      /* ON, weight = 10, max_diff = 0.1 */
int dvo_batch_set_geometric(dvo_batch* b, const dvo_geometric_config* cfg);       /* sensor-depth batches; from the next push on */
int dvo_batch_last_geometric(dvo_batch* b, dvo_geometric_record* rec);            /* [n_seq], host, synchronises */
int dvo_batch_last_geometric_log(dvo_batch* b, int seq, dvo_geometric_log* log);  /* host, synchronises */
/* ---- the geometric term with affine brightness compensation: sensor-depth batches only ------------------------------------------
 * dvo_batch_set_geometric_affine turns both terms on together (an RGB-D camera under auto-exposure): the two setters above keep
 * refusing each other, this call is the one way to the pair.  All arithmetic is float32 and IEEE, with no contraction beyond the
 * fmaf()s named.  The inputs are the geometric term's: pixel x of the TRACKED frame uses that frame's own depth, weight and gray I1.
 *   The photometric row is the compensated one on those inputs: c = fmaf(a, I1, b);  r = I2 - c;  rw = r * wgt, slots 0..28, and
 *   n_valid, the residual and the stop tests as under dvo_batch_set_affine_brightness.
 *   The brightness moments are the ones without robust weights (M1, M2, M11, M12, N = n_valid) over the same contributing pixels,
 *   reduced in their own fixed order; the closed form and its guards are unchanged.
 *   The geometric row does not see (a, b): it is dvo_batch_set_geometric's bit for bit (slots 0..26, S29, S30, the same gates), and a
 *   pixel without a geometric row adds exact zeros.
 *   DVO_AFFINE_ESTIMATE runs the priming pair on the coarsest level at the start pose; the pair writes the affine entry and nothing
 *   else: no pose, no track log, no geometric record or log, no affine log slot.
 * Anchors: (a, b) = (1, 0) makes every sum the geometric term's alone, bit for bit; weight = 0 makes the 27 sums and the moments
 * the affine estimator's on own-depth inputs, bit for bit.
 * geo->mode must be DVO_GEOMETRIC_ON and aff->mode DVO_AFFINE_ESTIMATE or DVO_AFFINE_GIVEN.  Takes effect from the next push; the
 * call may be repeated to reconfigure, whatever the state of the two terms.  Turning off and reading back use what exists:
 * dvo_batch_set_geometric(OFF / NULL) leaves the affine family on, dvo_batch_set_affine_brightness(OFF / NULL) leaves the geometric
 * family on, dvo_batch_set_affine_rows gives the rows of the GIVEN mode, and dvo_batch_last_affine, dvo_batch_last_affine_log,
 * dvo_batch_last_geometric and dvo_batch_last_geometric_log read what they document: both terms are ready after a composed push.
 * While on, every level runs launch pairs (k_track_gn_zab + k_gn_solve_zab).
 * Errors, returned before anything is enqueued: a NULL handle or a NULL config, either config failing its own setter's checks, a
 * mode that is off, a mono batch, robust weights on (dvo_batch_set_robust_weights keeps refusing while the geometric term is on)
 * -> DVO_ERR_BAD_ARGUMENT.  Robust weights with the geometric term, mono batches and dvo_vo handles are out of scope. */
int dvo_batch_set_geometric_affine(dvo_batch* b, const dvo_geometric_config* geo, const dvo_affine_config* aff);
/* ---- step control: damped Gauss-Newton with step acceptance (both batch kinds) ---------------------------------------------------
 * By default the tracker takes every Gauss-Newton step it computes.  dvo_batch_set_step_control makes every later push / call compare
 * the cost at the new pose with the cost at the old one, keep the better pose and damp when it got worse (Levenberg-Marquardt).  The
 * per-pixel kernels do not change: every evaluation is the plain one, at the pose the sequence holds.  Decisions are float32 and
 * integer, IEEE, no contraction, so a host replica has the device's bits.
 * Per sequence a dvo_lm_entry lives on the device: the accepted twist xi with its Tc = exp(xi) in double and pose = float(exp(-xi)),
 * the accepted evaluation's 21 + 6 sums, sum_r2, n_valid and residual ((float)sum_r2 / (float)n_valid, -1 without pixels), and lambda.
 * Every tracking call starts with lambda = lambda0; lambda carries across levels.  Each iteration of a level evaluates the pose the
 * sequence holds; with residual and n_valid of that evaluation, and residual_acc and n_acc of the entry, the solve then does:
 *   1. Decide.  The first evaluation of a level is DVO_LM_FIRST: accepted unconditionally, lambda unchanged.  Otherwise
 *      DVO_LM_ACCEPT iff n_valid > 0 && (float)n_valid >= min_valid_fraction * (float)n_acc && residual <= residual_acc (a NaN
 *      residual rejects, a tie accepts), else DVO_LM_REJECT.  FIRST and ACCEPT store this evaluation as the entry; ACCEPT sets
 *      lambda = lambda * lambda_down; REJECT keeps the entry and sets lambda = fminf(fmaxf(lambda, lambda_floor) * lambda_up, lambda_max).
 *   2. Step.  From the entry, whichever evaluation it now holds: the six diagonal sums of H times 1.0 + (double)lambda, the 6x6 solve
 *      of the plain tracker, trial = log(exp(xi_acc) exp(upd)) by the plain tracker's pose update on the entry's Tc.  With n_acc == 0
 *      the update is zero.
 *   3. Stop tests.  fixed_iterations > 0: the level runs that many evaluations.  Otherwise it stops when |upd| < min_update, when
 *      residual_acc < min_residual, or after max_iterations evaluations.  In either mode a non-finite update (a component of upd or of
 *      the composed twist that is not finite) also ends the level.  A sequence that stays active holds the trial pose; a sequence that
 *      stops holds the accepted pose.
 * A level therefore always ends on an evaluated, accepted pose, and on each level the accepted residuals never increase.  The step
 * computed in the iteration that stops is not taken: with min_residual above a level's first residual the level ends on the pose it
 * started from, so step control is meant to run with min_residual = 0 (stop on the update norm).
 * The track log keeps its meaning per evaluation (residual, n_valid of the evaluation; xi_update, update_norm of the step computed in
 * that iteration); xi_after is the pose the sequence holds after the iteration.  The quality record (dvo_batch_set_track_quality)
 * receives the accepted sums of the finest level: H, g, sum_r2, n_valid, residual and the covariance describe the returned pose.
 * Anchor: with lambda0 = 0, inputs that never reject and a level started at the same pose, every evaluated pose and every logged
 * sum of that level equals the plain batch's bit for bit; only the pose the level ends on is one step behind.
 * Takes effect from the next push / call; cfg == NULL or mode == DVO_LM_OFF goes back to the plain launches, and a batch that never
 * calls this runs exactly the launches it always ran.  While on, every level runs launch pairs (k_track_gn + k_gn_solve_lm) whatever
 * track_fused_tiles, gn_use_lds_patch and track_single_launch say.
 * dvo_batch_last_step_control: rec[n_seq] (host, synchronises) -- per sequence of the last push / call the FIRST, ACCEPT and REJECT
 * decisions counted over all levels, the lambda it ended on and the accepted residual of the finest level; all zeros for a sequence
 * that did not track.  dvo_batch_last_step_control_log: per level and logged iteration, indexed like dvo_track_log, the lambda that
 * iteration's solve used (after its decision) and the decision; empty (n_iter all 0) for a sequence that did not track.
 * Errors, returned before anything is enqueued: a NULL handle, struct_size != sizeof(dvo_lm_config), a mode outside the set, a lambda
 * parameter that is not finite or negative, lambda_up <= 1, lambda_down outside (0, 1], lambda_floor <= 0, lambda_max < lambda_floor,
 * min_valid_fraction outside [0, 1], robust weights, the median scale, affine brightness or the geometric term on ->
 * DVO_ERR_BAD_ARGUMENT; while step control is on, dvo_batch_set_robust_weights, dvo_batch_set_robust_median,
 * dvo_batch_set_affine_brightness, dvo_batch_set_geometric and dvo_batch_set_geometric_affine refuse to turn their term on.  A read
 * before a push / call that ran with step control on -> DVO_ERR_NOT_READY.  Step control together with those terms, and dvo_vo
 * handles, are out of scope. */
#define DVO_LM_OFF 0
#define DVO_LM_ON  1
#define DVO_LM_FIRST  1
#define DVO_LM_ACCEPT 2
#define DVO_LM_REJECT 3
typedef struct dvo_lm_config {
    int   struct_size;          /* sizeof(dvo_lm_config) */
    int   mode;                 /* DVO_LM_* */
    float lambda0;              /* >= 0: lambda at the start of every tracking call */
    float lambda_up;            /* > 1 */
    float lambda_down;          /* (0, 1] */
    float lambda_floor;         /* > 0: a rejected step raises lambda from at least this */
    float lambda_max;           /* >= lambda_floor */
    float min_valid_fraction;   /* [0, 1]: an evaluation with fewer pixels than this fraction of the accepted one's is rejected */
} dvo_lm_config;
typedef struct dvo_lm_record {
    int   n_first, n_accepted, n_rejected;   /* decisions of the last push / call, all levels */
    float lambda;                            /* the lambda the sequence ended on */
    float residual;                          /* the accepted residual of the finest level */
} dvo_lm_record;
typedef struct dvo_lm_log {
    int   struct_size;    /* sizeof(dvo_lm_log), set by the caller */
    int   levels;
    int   n_iter[DVO_MAX_LEVELS];
    float lambda[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];     /* the lambda the iteration's solve used */
    int   decision[DVO_MAX_LEVELS][DVO_MAX_ITERATIONS];   /* DVO_LM_FIRST / ACCEPT / REJECT */
} dvo_lm_log;
typedef struct dvo_lm_entry {
    double Tc[12];        /* exp(xi) in double: R row major, then t */
    double H[21];         /* the accepted evaluation's sums, as dvo_gn_result */
    double g[6];
    double sum_r2;
    float  xi[6];         /* the accepted twist */
    float  pose[12];      /* float(exp(-xi)): R row major, then t */
    int    n_valid;
    float  residual;
    float  lambda;
    int    reserved;
} dvo_lm_entry;
void dvo_lm_config_default(dvo_lm_config* cfg);   /* ON, lambda0 1, up 4, down 0.5, floor 1e-4, max 1e6, min_valid_fraction 0.5 */
int dvo_batch_set_step_control(dvo_batch* b, const dvo_lm_config* cfg);            /* both kinds; from the next push / call on */
int dvo_batch_last_step_control(dvo_batch* b, dvo_lm_record* rec);                /* [n_seq], host, synchronises */
int dvo_batch_last_step_control_log(dvo_batch* b, int seq, dvo_lm_log* log);      /* host, synchronises */
/* Profile of the mapping stages (cfg.profile = 1): hipEvent-bracketed durations on the handle's stream, summed over the frames
 * since the last reset.  depth_update = k_age_table + k_depth_update (Mapper::update), regularize = k_regularize_redecimate
 * (Mapper::regularize + Frame::updateDepth*), propagate = the three k_propagate_* passes (Mapper::propagate). */
typedef struct dvo_map_profile {
    uint64_t frames;
    double   depth_update_ms, regularize_ms, propagate_ms;
    uint64_t update_window_pixels;   /* pixels one k_depth_update launch covers (window of mapper.cpp:90 x n_seq) */
    uint64_t map_pixels;             /* top-level pixels x n_seq (one k_regularize_redecimate launch) */
} dvo_map_profile;
int dvo_batch_profile_mapping(dvo_batch* b, dvo_map_profile* out, int reset);

/* ------------------------------------------------------------------------------------------------
 * Operator level (host pointers): each runs the corresponding HIP kernel once.  Used by the parity
 * tests and reusable on their own.  `dev` is the HIP device ordinal.
 * ------------------------------------------------------------------------------------------------ */
/* Convert::cullImage, src/core/convert.cpp:7-20.  dst is (w>>times) x (h>>times). */
int dvo_op_cull_image(int dev, const float* src, int w, int h, int times, float* dst);
/* Convert::gradiate, src/core/convert.cpp:41-75 */
int dvo_op_gradient(int dev, const float* img, int w, int h, int xdir, float* out);
/* Transform::warpImage, src/core/transform.cpp:35-51 */
int dvo_op_warp_image(int dev, const float xi[6], const float* gray, const float* depth, int w, int h,
                      const float K[9], float* out);
/* Frame pyramid, src/system/frame.cpp:16-37: fills gray/depth/sigma level buffers (coarsest first, each
 * (w>>culls>>(levels-1-i)) x (h>>culls>>(levels-1-i))), any of depth/sigma may be NULL. */
int dvo_op_pyramid(int dev, const float* gray, const float* depth, const float* sigma, int w, int h,
                   int levels, int culls, float* const gray_out[], float* const depth_out[], float* const sigma_out[]);
/* The batched pyramid build of the push entry points, run once on host pointers: n_seq frames through the engine's own build (the
 * argument blocks, the fused weight maps, the plan's copy-forward and the launch decision are the ones a batch uses), every map of
 * every level returned, and the kernel that ran reported by the launcher that chose it.
 * Input, one of:
 *   float maps   gray [n_seq][rows][w], optionally depth AND sigma (both or neither), rgb = NULL
 *   raw frames   rgb [n_seq][rows][w][channels] u8 with channels 1 (gray), 3 (R,G,B) or 4 (R,G,B,A), optionally depth16 [n_seq][rows][w]
 *                u16 and depth_scale (0 = 1/5000); gray = depth = sigma = NULL.  Converted as the raw push entry points convert:
 *                gray = (float)g8 * (float)(1/255) with g8 the byte (1 channel) or (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 in
 *                integers (dvo_op_ingest's luma); with depth16: depth = (float)d16 * depth_scale, sigma = 0.1f where d16 > 0 else 1.0f,
 *                gray = DVO_INVALID where d16 == 0.
 * rows = h, or h >> culls with DVO_PYRAMID_ROWS_DECIMATED: the buffers hold only rows 0, 2^culls, 2 * 2^culls ... of each frame (what
 * the host push forms upload; needs culls > 0 and h a multiple of 2^culls).
 * Output: level l (0 = coarsest) of a map is [n_seq][h_l][w_l] with w_l = (w >> culls) >> (levels - 1 - l), h_l likewise, and holds
 * pixel (x << s, y << s) of the converted input, s = culls + (levels - 1 - l), with NaN and every value <= DVO_INVALID replaced by
 * DVO_INVALID -- except the top level at culls = 0, which is the input unchanged.  wgt = step_l / min(max(sigma, sigma_min),
 * sigma_max), one float division, with step_l = step_level1 / step_level2 for l = 1 / 2 and step_default otherwise (cfg, or the
 * defaults for NULL).  The build keeps sigma (keep_sigma = true), so with depth all four maps are written whether or not
 * DVO_PYRAMID_FORCE_WEIGHT_MAPS is set (the flag clears the frame sets' constant-weight shortcut, as DVO_WEIGHT_MAPS does for a
 * batch).  A map the build does not write (depth, sigma and wgt without depth) comes back as words of 0xffffffff: the frame sets are
 * filled with them before the build, so an element the build should have written and did not shows too.
 * Any of the four output arrays, and any entry, may be NULL.
 * DVO_PYRAMID_SPLIT asks for the split build (k_pyramid_raw4_coarse + k_pyramid_raw4_rest, each on a stream of its own as in a
 * batch); where it is not possible the single kernel runs, which is no error: *ran says what ran.
 * seq_action != NULL: a planned build.  The first frames are built plainly into a set A; then the second frames (gray2 ... / rgb2,
 * depth16_2: the same kind, shape and optional maps as the first) are built into a set B with the EFFECTIVE per-sequence actions
 * seq_action[n_seq] (DVO_SEQ_SKIP / TRACK / RESTART) and A as the set to copy forward from, and B is returned: a SKIP sequence's maps
 * are A's top-level values decimated as above and A's wgt, and its second input frame is not read.  *ran is B's build.
 * ran->kind: DVO_PYRAMID_KERNEL_SCALAR k_pyramid<plan>; _RAW4 k_pyramid_raw4<culls, plan>; _SPLIT k_pyramid_raw4_coarse<culls> +
 * k_pyramid_raw4_rest<culls>; _REMAP the undistorting kernels (never from this op).  culls is 0 where the kernel has no such instance.
 * Errors, returned before anything is queued -> DVO_ERR_BAD_ARGUMENT: NULL args, a struct_size that is not sizeof, n_seq < 1, a
 * geometry dvo_batch_create refuses, both or neither of gray and rgb, depth without sigma or the reverse, float maps beside raw ones,
 * channels not 1 / 3 / 4, a depth_scale that is negative or not finite, unknown flag bits, DVO_PYRAMID_ROWS_DECIMATED where rows
 * cannot be decimated, second frames without seq_action or of another kind than the first, seq_action without second frames, an
 * action that is not 0 / 1 / 2. */
#define DVO_PYRAMID_KERNEL_SCALAR 0
#define DVO_PYRAMID_KERNEL_RAW4   1
#define DVO_PYRAMID_KERNEL_SPLIT  2
#define DVO_PYRAMID_KERNEL_REMAP  3
/* the kernels of a handle with a photometric calibration (dvo_batch_set_photometric; never from dvo_op_pyramid_frames):
 * k_pyramid_raw4_photo<2, plan>, k_pyramid_photo<plan, false> and, with lens undistortion, k_pyramid_photo<plan, true> */
#define DVO_PYRAMID_KERNEL_PHOTO_RAW4   4
#define DVO_PYRAMID_KERNEL_PHOTO_SCALAR 5
#define DVO_PYRAMID_KERNEL_PHOTO_REMAP  6
#define DVO_PYRAMID_ROWS_DECIMATED    1
#define DVO_PYRAMID_FORCE_WEIGHT_MAPS 2
#define DVO_PYRAMID_SPLIT             4
typedef struct dvo_pyramid_kernel {
    int kind, culls, plan;
} dvo_pyramid_kernel;
typedef struct dvo_pyramid_frames_args {
    int struct_size;                      /* sizeof(dvo_pyramid_frames_args) */
    int n_seq, w, h, levels, culls, flags;
    int channels;                         /* raw frames: 1, 3 or 4 */
    float depth_scale;                    /* raw frames with depth16: 0 = 1/5000 */
    const float *gray, *depth, *sigma;    /* float maps */
    const uint8_t* rgb;                   /* raw frames */
    const uint16_t* depth16;
    const uint8_t* seq_action;            /* [n_seq], or NULL: one plain build */
    const float *gray2, *depth2, *sigma2; /* the second frames of a planned build */
    const uint8_t* rgb2;
    const uint16_t* depth16_2;
} dvo_pyramid_frames_args;
int dvo_op_pyramid_frames(int dev, const dvo_config* cfg, const dvo_pyramid_frames_args* args, float* const gray_out[],
                          float* const depth_out[], float* const sigma_out[], float* const wgt_out[], dvo_pyramid_kernel* ran);
/* dvo_op_pyramid_frames with the gray pyramid filtered as dvo_batch_set_pyramid_filter states (same arguments, planned builds
 * included; the first frames of a planned build are filtered too).  filter = DVO_PYRAMID_FILTER_NONE: dvo_op_pyramid_frames, byte
 * for byte.  With a filter: ran->kind = DVO_PYRAMID_KERNEL_FILTER (k_pyramid_filter_top<culls, raw, plan, wide> and one
 * k_pyramid_filter_down<plan> per level below the top), ran->culls = culls and ran->plan = PLAN | WIDE << 1 | RAW << 2 (WIDE: the
 * source footprint is staged with 16-byte loads -- 1-channel bytes with w a multiple of 16, or float maps with w a multiple of 4,
 * culls > 0); DVO_PYRAMID_ROWS_DECIMATED, DVO_PYRAMID_SPLIT, culls > 2 and a filter outside the set -> DVO_ERR_BAD_ARGUMENT. */
#define DVO_PYRAMID_KERNEL_FILTER 7
int dvo_op_pyramid_frames_filtered(int dev, const dvo_config* cfg, const dvo_pyramid_frames_args* args, int filter,
                                   float* const gray_out[], float* const depth_out[], float* const sigma_out[],
                                   float* const wgt_out[], dvo_pyramid_kernel* ran);
/* Debug readers of a mono batch's photometric calibration (host memory; both synchronise the batch's stream).
 * photometric_gain: the gain table sequence `seq` reads, [h_top][w_top]: 1.0f / vignette at each kept pixel's source, -1.0f where the
 * pixel is masked (vignette not finite or <= 0) or the remap's index is -1.  DVO_ERR_NOT_READY without a calibration.
 * last_pyramid_kernel: what the last frame build of the batch launched (DVO_ERR_NOT_READY before the first frame). */
int dvo_debug_batch_photometric_gain(dvo_batch* b, int seq, float* gain /* [h_top][w_top] */);
int dvo_debug_batch_last_pyramid_kernel(dvo_batch* b, dvo_pyramid_kernel* ran);
/* Track::optimize, src/track/optimize.cpp:10-99: one Gauss-Newton step on one level.
 * H = upper triangle of sum J^T J (21), g = sum J^T (w r) (6).  mask (optional, w*h bytes). */
typedef struct dvo_gn_result {
    double H[21];
    double g[6];
    double sum_r2;
    int    n_valid;
    float  xi_update[6];
    float  residual;
    float  xi_next[6];   /* se3::concatenate(xi, xi_update), tracker.cpp:46 */
} dvo_gn_result;
int dvo_op_gn_step(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray,
                   const float* ref_depth, const float* ref_sigma, int w, int h, const float K[9],
                   const float xi[6], int level, dvo_gn_result* out, uint8_t* mask);
/* dvo_op_gn_step with robust residual weights (dvo_batch_set_robust_weights): every contributing pixel weighted by rho of (kind,
 * param, s2); kind = DVO_ROBUST_NONE, or an s2 that is not finite and > 0, is plain.  No mask: it is dvo_op_gn_step's. */
int dvo_op_gn_step_robust(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray,
                          const float* ref_depth, const float* ref_sigma, int w, int h, const float K[9],
                          const float xi[6], int level, int kind, float param, float s2, dvo_gn_result* out);
/* dvo_op_gn_step_robust through the median scale's pair (dvo_batch_set_robust_median: k_track_gn_md + k_gn_solve_md), run once: the
 * same weighted sums, plus counts[256] of the contributing pixels' |r|, the median bin the solve selected (-1 where no pixel
 * contributed) and next_s2, the s2 of the entry it wrote (+inf: plain), with floor2 = 0. */
int dvo_op_gn_step_robust_median(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray,
                                 const float* ref_depth, const float* ref_sigma, int w, int h, const float K[9],
                                 const float xi[6], int level, int kind, float param, float s2,
                                 dvo_gn_result* out, uint32_t counts[256], int* median_bin, float* next_s2);
/* dvo_op_gn_step_robust with affine brightness compensation (dvo_batch_set_affine_brightness): the pair run once with the entry (a, b)
 * ((1, 0) unless finite with a > 0).  moments = (N, M1, M2, M11, M12) in double, N being M0 with robust weights and n_valid with kind =
 * DVO_ROBUST_NONE; next_ab = the entry the solve writes from them under the guards min_pixels = 64, min_contrast = 1e-3, gain range
 * [0.25, 4] ((a, b) itself where a guard fails). */
int dvo_op_gn_step_affine(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray,
                          const float* ref_depth, const float* ref_sigma, int w, int h, const float K[9],
                          const float xi[6], int level, int kind, float param, float s2, float a, float b,
                          dvo_gn_result* out, double moments[5], float next_ab[2]);
/* The pair with the geometric term (dvo_batch_set_geometric) run once on host pointers: obj_* are the tracked frame's gray, depth and
 * sigma, ref_* the reference's gray and depth.  sums = (n_geo, S29) in double. */
int dvo_op_gn_step_geometric(int dev, const dvo_config* cfg, const float* obj_gray, const float* obj_depth,
                             const float* obj_sigma, const float* ref_gray, const float* ref_depth, int w, int h,
                             const float K[9], const float xi[6], int level, float weight, float max_diff,
                             dvo_gn_result* out, double sums[2]);
/* The pair with both terms (dvo_batch_set_geometric_affine) run once on host pointers: dvo_op_gn_step_geometric's inputs with the
 * entry (a, b) of dvo_op_gn_step_affine, kind DVO_ROBUST_NONE.  sums = (n_geo, S29); moments = (n_valid, M1, M2, M11, M12); next_ab
 * under dvo_op_gn_step_affine's guards. */
int dvo_op_gn_step_geometric_affine(int dev, const dvo_config* cfg, const float* obj_gray, const float* obj_depth,
                                    const float* obj_sigma, const float* ref_gray, const float* ref_depth, int w, int h,
                                    const float K[9], const float xi[6], int level, float weight, float max_diff,
                                    float a, float b, dvo_gn_result* out, double sums[2], double moments[5], float next_ab[2]);
/* Tracker::track, src/track/tracker.cpp:22-85, on full-resolution frames (pyramids built on device). */
int dvo_op_track(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray,
                 const float* ref_depth, const float* ref_sigma, int w, int h, const float K[9],
                 int levels, int culls, float xi_out[6], dvo_track_log* log);
/* Map::Implement::propagate, src/map/implement.cpp:217-256 */
int dvo_op_propagate(int dev, const float* ref_depth, const float* ref_sigma, const float* ref_age, int w, int h,
                     const float xi[6], const float K[9], float* depth, float* sigma, float* age);
/* Map::Implement::regularize, src/map/implement.cpp:156-180 */
int dvo_op_regularize(int dev, const float* depth, const float* sigma, int w, int h, float* out);
/* Map::Mapper::update, src/map/mapper.cpp:76-137, against n_hist keyframes (oldest first, the last one is the
 * reference keyframe whose depth/sigma/age are updated in place).  All maps are top-level w x h.
 * hist_gray[i], hist_xi[i] (6 floats each) describe keyframe i. */
int dvo_op_depth_update(int dev, const dvo_config* cfg, int n_hist, const float* const hist_gray[],
                        const float* hist_xi, const float* obj_gray, const float obj_xi[6],
                        const float obj_rel_xi[6], int obj_id, const float K[9], int w, int h,
                        float* ref_depth, float* ref_sigma, float* ref_age, int* valid_updates);
/* Mapper::update as a MONO BATCH runs it (parity op): the !need branch of one call of dvo_batch_odometrize -- k_age_table over each
 * sequence's keyframe ring, then k_depth_update, or k_depth_update_cam with per_camera -- for n_seq sequences whose state is given
 * instead of tracked.  The op creates a mono batch of n_seq sequences for w x h frames (3 levels, 2 culls: maps are mw x mh = (w >> 2)
 * x (h >> 2)) with ring size `ring` and K ([9] at FULL resolution, or [n_seq][9] with per_camera != 0: the batch's own per-sequence
 * tables), fills its buffers and queues what the batch queues.  Per sequence q:
 *   n_total[q] >= 1   keyframes created so far.  The newest n_hist = min(n_total, ring) are retained: kf_gray[q][i] (mw x mh top-level
 *                     gray) and kf_xi[q][i] (world twist), i = 0 .. n_hist - 1 OLDEST FIRST (entries i >= n_hist are not read), are
 *                     stored at ring slot (n_total - n_hist + i) % ring, as the batch's commits leave them.
 *   obj_gray[q], obj_xi[q], obj_rel_xi[q], frame_id[q]   the tracked frame: top-level gray, world twist, twist relative to the newest
 *                     keyframe, frame id (the reset depth's hash key).
 *   need[q]           0 or 1: 1 = the sequence creates a keyframe on this frame and takes no part: its maps come back as given.
 *   depth, sigma, age [n_seq][mh][mw], in place: the newest keyframe's top-level maps.
 * A pixel whose age points past the ring (n_hist - 1 - (int)age < 0) is searched against the oldest retained keyframe and counted in
 * clamped[q] (dvo_mono_stats::clamped_pixels' contract); a negative age (>= n_hist) leaves the pixel alone.  valid_updates[q] = the accepted
 * updates.  Both arrays are written for every sequence (0 for need = 1) and may be NULL.  cfg: crop_enable and rng_seed are used.
 * Errors, returned before anything is queued -> DVO_ERR_BAD_ARGUMENT: NULL args, a struct_size that is not sizeof, n_seq < 1, a NULL
 * input or map, a geometry or K dvo_batch_create_mono[_cameras] refuses (w or h < 64, ring outside 1 .. 64, K not finite or fx, fy
 * <= 0), n_total < 1, need not 0 or 1. */
typedef struct dvo_depth_update_batch_args {
    int struct_size;                 /* sizeof(dvo_depth_update_batch_args) */
    int n_seq, w, h, ring, per_camera;
    const float* K;                  /* [9], or [n_seq][9] with per_camera */
    const int* n_total;              /* [n_seq] */
    const float* kf_gray;            /* [n_seq][ring][mh][mw] */
    const float* kf_xi;              /* [n_seq][ring][6] */
    const float* obj_gray;           /* [n_seq][mh][mw] */
    const float* obj_xi;             /* [n_seq][6] */
    const float* obj_rel_xi;         /* [n_seq][6] */
    const int* need;                 /* [n_seq] */
    const int* frame_id;             /* [n_seq] */
} dvo_depth_update_batch_args;
int dvo_op_depth_update_batch(int dev, const dvo_config* cfg, const dvo_depth_update_batch_args* args, float* depth, float* sigma,
                              float* age, int* valid_updates, int* clamped);
/* math::se3 (src/math/se3.cpp:70-131) evaluated ON THE DEVICE (the tracker's pose chain runs there) */
int dvo_op_se3_exp(int dev, const float xi[6], float T[16]);
int dvo_op_se3_log(int dev, const float T[16], float xi[6]);
int dvo_op_se3_concatenate(int dev, const float a[6], const float b[6], float out[6]);
/* The tracker's serial double-precision chain, piece by piece, ON THE DEVICE for n cases at once (parity op: the tests hold it to a
 * multi-precision reference).  Every value travels as a double (exact for the float ones); rows per case:
 *   op 0  se3 exp in double            in xi[6]                          out R[9] t[3], before any rounding to float
 *   op 1  se3 log in double            in R[9] t[3]                      out xi[6]
 *   op 2  concatenate                  in a[6] b[6] (float values)       out xi[6] (float values)
 *   op 3  one pose update of the       in xi[6] upd[6] (float values)    out ok (1 or 0), xi'[6], exp(xi') as R[9] t[3] in double,
 *         tracker from the state                                             float(exp(-xi')) as R[9] t[3]; ok = 0 (a non-finite
 *         of xi                                                              result) leaves all three as they were for xi
 *   op 4  the 6x6 solve x = H^+ g      in H[21] (upper triangle by rows) g[6]   out x[6] (float values), 1 if the pseudo-inverse ran
 *   op 5  the Jacobi eigensolver       in H[21]                          out eigenvalues[6] (unsorted), V[36] (columns, row major)
 * DVO_ERR_BAD_ARGUMENT for a null pointer, n < 1 or another op. */
int dvo_op_pose_algebra(int dev, int op, int n, const double* in, double* out);
/* The serial tail of the step-control solve (dvo_batch_set_step_control: k_gn_solve_lm's decide / step / stop rules) ON THE DEVICE for
 * n cases at once, on given sums: sums[n][29] (H[21], g[6], sum_r2, n_valid as a double) of an evaluation at the twist xi_eval[n][6],
 * against the entry entry_in[n] (of which xi, Tc, pose, the sums, n_valid, residual and lambda are read as they are).  level_first:
 * the evaluation is a level's first; it_prev: the iterations the level has done before it (ignored with level_first); the stop
 * constants are dvo_config's.  Out: entry_out[n], update[n][6] (the step computed from the entry), xi_next[n][6] (the pose the
 * sequence holds after the iteration), decision[n] (DVO_LM_*) and active[n] (1: the level goes on).  cfg as validated by
 * dvo_batch_set_step_control, mode DVO_LM_ON.  DVO_ERR_BAD_ARGUMENT for a null pointer, n < 1 or a config that is refused there. */
int dvo_op_lm_step(int dev, int n, const double* sums, const float* xi_eval, const dvo_lm_entry* entry_in, const dvo_lm_config* cfg,
                   int level_first, int it_prev, int max_iterations, int fixed_iterations, float min_update, float min_residual,
                   dvo_lm_entry* entry_out, float* update, float* xi_next, int* decision, int* active);

/* ------------------------------------------------------------------------------------------------
 * Dataset front-end: what src/core/loader.cpp + include/core/loader.hpp do with OpenCV.
 * ------------------------------------------------------------------------------------------------ */
/* PNG reader (cv::imread(IMREAD_UNCHANGED), loader.cpp:61-73,149-160): non-interlaced 8/16-bit gray, gray+alpha, RGB, RGBA.
 * pixels: row-major interleaved channels in FILE order (R,G,B[,A]); 16-bit samples as host-endian uint16. */
int dvo_png_info(const char* path, int* width, int* height, int* channels, int* bit_depth);
int dvo_png_read(const char* path, void* pixels, size_t capacity_bytes);
typedef struct dvo_dataset dvo_dataset;
/* TUM RGB-D directory: rgb.txt + depth.txt associated by nearest timestamp (|dt| <= max_dt, default 0.02 s),
 * optional groundtruth.txt (tx ty tz qx qy qz qw). */
int dvo_dataset_open_tum(const char* dir, double max_dt, dvo_dataset** out);
/* The reference's list files (include/core/loader.hpp:38-47,87-98): "file" or "rgb depth" per line; NULL = dir/info.txt */
int dvo_dataset_open_list(const char* dir, const char* list_file, dvo_dataset** out);
int dvo_dataset_size(const dvo_dataset* d);
int dvo_dataset_entry(const dvo_dataset* d, int i, double* timestamp, char* rgb_path, char* depth_path, int path_capacity,
                      float gt_pose7[7]);
int dvo_dataset_close(dvo_dataset* d);
/* Device-side conversion of raw sensor frames (k_ingest): gray = BGR2GRAY(u8)/255 (loader.cpp:55-60,137-147), depth =
 * u16 * depth_scale (1/5000), sigma = sigma_valid where depth > 0 else sigma_invalid, gray = INVALID where depth == 0 when
 * invalidate_gray (what Transform::mapDepthtoGray leaves, src/core/transform.cpp:60-76).  depth16 may be NULL (gray only). */
int dvo_op_ingest(int dev, const uint8_t* rgb, int channels, const uint16_t* depth16, int w, int h, float depth_scale,
                  float sigma_valid, float sigma_invalid, int invalidate_gray, float* gray, float* depth, float* sigma);
/* odometrizeUsingDepth fed with raw frames (u8 gray/RGB/RGBA + u16 depth): converted on the device, 1.5 instead of 3.7 MB/frame */
int dvo_vo_odometrize_depth_raw(dvo_vo* vo, const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale,
                                float T_rel[16]);
/* Loader::getNormalizedUndistortedImages (loader.cpp:15-42): radial-tangential undistortion D = (k1,k2,p1,p2,k3), nearest
 * remap, INVALID border. */
int dvo_op_undistort(int dev, const float* src, int w, int h, const float K[9], const float D[5], float* dst);

/* ------------------------------------------------------------------------------------------------
 * Keyframe store / checkpoint and debug views (row 4).
 * ------------------------------------------------------------------------------------------------ */
/* Dump / restore the whole FrameHistory (include/system/frame.hpp:146-188): per keyframe id, poses, the gray pyramid and the
 * top-level depth / sigma / age.  dvo_vo_load needs a handle created with the same K and frame size; it replaces the history. */
int dvo_vo_save(const dvo_vo* vo, const char* path);
int dvo_vo_load(dvo_vo* vo, const char* path);
/* 0 = keep every keyframe (the reference); N > 0 = keep the newest N (a pixel born in a dropped keyframe then matches
 * against the oldest retained one -- the reference's commented-out `age = std::min(age, 2)`, src/map/mapper.cpp:100). */
int dvo_vo_set_history_limit(dvo_vo* vo, int max_keyframes);
/* False-colour views of src/core/draw.cpp:7-100 as RGB bytes [h][w][3]: mode 0 gray (INVALID blue), 1 depth (hue) with
 * optional sigma (value) in b, 2 sigma, 3 age, 4 gradient.  No GUI: write them with dvo_ppm_write. */
int dvo_op_visualize(int dev, int mode, const float* a, const float* b, int w, int h, uint8_t* rgb);
int dvo_ppm_write(const char* path, const uint8_t* rgb, int w, int h);

/* Device self-test: the kernels' correctly rounded reciprocal (v_rcp_f32 + two FMA corrections inside [2^-100, 2^100], IEEE
 * division elsewhere) against the IEEE division for all 2^32 float bit patterns.  mismatches must come back 0. */
int dvo_selftest_reciprocal(int device, uint64_t* fast_path_inputs, uint64_t* mismatches, uint32_t* first_bad_bits);
/* The regularize kernels' short square root (v_rsq_f32 + 4 operations) against sqrtf for every float in [2^-100, 2^100], and their
 * short division (the reciprocal above + 3 operations) against the IEEE quotient for b = 1.mb, mb = b_first + i * b_stride
 * (i < b_count), times ALL 2^23 mantissas of a in [1, 2); b_first = 0, b_stride = 1, b_count = 2^23 is every mantissa pair (minutes).
 * first_bad_pair = mb << 23 | ma.  mismatches must come back 0. */
int dvo_selftest_sqrt(int device, uint64_t* inputs, uint64_t* mismatches, uint32_t* first_bad_bits);
/* The double-precision sin / cos / atan2 kernels the device's SE(3) chain uses (polynomial kernels instead of the math library's
 * general-purpose routines) against that library on 2^24 arguments of their domain: largest relative differences (expected < 1e-15). */
int dvo_selftest_trig(int device, double* max_rel_sin, double* max_rel_cos, double* max_rel_atan2, uint64_t* samples);
int dvo_selftest_division(int device, uint32_t b_first, uint32_t b_stride, uint32_t b_count, uint64_t* pairs, uint64_t* mismatches,
                          uint64_t* first_bad_pair);

/* ------------------------------------------------------------------------------------------------
 * Trajectory evaluation / export.  Host side, double precision.
 * ------------------------------------------------------------------------------------------------ */
/* ATE: RMSE of |gt_i - (s R est_i + t)| after the optimal rigid (with_scale: similarity) alignment (Horn). xyz: [n][3] */
int dvo_eval_ate(int n, const float* est_xyz, const float* gt_xyz, int with_scale, double* rmse, double R_out[9],
                 double t_out[3], double* scale_out);
/* RPE over `delta` frames: RMSE of the translational part [m] and of the rotation angle [rad]; poses [n][16] row major */
int dvo_eval_rpe(int n, const float* est_T, const float* gt_T, int delta, double* trans_rmse, double* rot_rmse);
/* the correct rigid inverse (Convert::inversePose, src/core/convert.cpp:31-39, is wrong in the reference) */
int dvo_pose_inverse(const float T[16], float out[16]);
/* "timestamp tx ty tz qx qy qz qw" per line; timestamps may be NULL (frame index is written) */
int dvo_traj_write_tum(const char* path, int n, const double* timestamps, const float* T);

#ifdef __cplusplus
}
#endif
#endif
