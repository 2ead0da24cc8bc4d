// dvo_engine.h -- C++ host side of libdvo.so: device memory, pyramids, the batched tracker and the
// single-sequence VisualOdometry (tracking + mapping).  Mirrors the reference's classes:
//   System::Frame / Scene  -> FrameSet (n_seq frames, one buffer per pyramid level)   include/system/frame.hpp
//   Track::Tracker         -> Tracker                                                 src/track/tracker.cpp
//   Map::Mapper            -> Mapper functions on Keyframe                             src/map/mapper.cpp
//   System::VisualOdometry -> VisualOdometry                                           include/system/system.hpp
// There is NO CPU fallback: every entry point fails with DVO_ERR_NO_DEVICE / DVO_ERR_HIP without a GPU.
#pragma once
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime_api.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "dvo_kernels.h"

namespace dvo {

void set_error(const std::string& s);
const char* last_error();
int check_hip(hipError_t e, const char* what);
#define DVO_HIP(call)                                              \
    do {                                                           \
        int _st = ::dvo::check_hip((call), #call);                 \
        if (_st != DVO_OK) return _st;                             \
    } while (0)
#define DVO_TRY(call)                                              \
    do {                                                           \
        int _st = (call);                                          \
        if (_st != DVO_OK) return _st;                             \
    } while (0)

struct DevBuf {  // RAII hipMalloc (or a view of memory somebody else owns: adopt())
    void* p = nullptr;
    size_t bytes = 0;
    bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n);
    void adopt(void* mem, size_t n) { release(); p = mem; bytes = n; owned = false; }
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Two pinned host blocks used alternately to stage small host tables (actions, intrinsics, start-pose rows) for a copy in stream
// order: the caller fills the block acquire() hands out and commit() queues its copy, so the call returns while the copy is pending
// and the block is reused two calls later, once its event says the copy has read it.
// Release order, for this and every helper that owns host staging (SeqPlan, HostStage): the owner's destructor calls release(stream)
// BEFORE it destroys the stream, which drains the stream, waits for the staged copies and then frees.  The member destructor runs
// after the owner's body, when the stream may be gone: it calls release(nullptr), which touches no stream, waits on the helper's own
// events only and does nothing after an explicit release.
struct PinnedPair {
    void* h[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};   // the copy out of h[i] has been read
    bool staged[2] = {false, false};
    int slot = 0;                            // the block the next acquire() hands out
    PinnedPair() = default;
    PinnedPair(const PinnedPair&) = delete;
    PinnedPair& operator=(const PinnedPair&) = delete;
    ~PinnedPair() { release(nullptr); }
    int alloc(size_t bytes);                                   // on first use; later calls do nothing
    int acquire(void** host);                                  // the next block, once the copy of two calls ago has read it
    int commit(void* dst_dev, size_t bytes, hipStream_t s);    // the block acquired last -> dst_dev, in stream order
    void release(hipStream_t s);
};

// Host rows that every later push / call reads (the robust weights' GIVEN scales, the GIVEN (a, b) rows, the start poses): either the
// caller's own device pointer, or host rows copied now into pinned staging and from there, in stream order, into `dev`.
struct HostRows {
    DevBuf dev;                   // where staged rows land (PoseGuess: a view of the rows inside its own block, DevBuf::adopt)
    PinnedPair stage;             // pinned staging of host rows
    const float* src = nullptr;   // the rows every later push / call reads (device memory); nullptr: none
    // rows: `bytes` of host memory (copied before the call returns), or with on_device device memory read in stream order; nullptr clears
    int set(const float* rows, bool on_device, size_t bytes, hipStream_t s);
    void clear() { src = nullptr; }
    void release(hipStream_t s) { stage.release(s); }   // (PinnedPair's release order)
};

// Device memory for the keyframes of one dvo_vo handle: FrameHistory grows by one Frame per keyframe (frame.hpp:151-157), and a hipMalloc
// per map of every new keyframe costs more than tracking a frame.  Blocks of one keyframe's size are cut from slabs of 16 and recycled
// when a keyframe is dropped (dvo_vo_set_history_limit).
struct KeyframePool {
    size_t block_bytes = 0;
    std::vector<std::unique_ptr<DevBuf>> slabs;
    std::vector<void*> free_blocks;
    int take(size_t bytes, void** out);
    void give(void* blk) { free_blocks.push_back(blk); }
};

struct Geometry {  // pyramid shape of Frame(gray, K, levels, culls): frame.hpp:91-117, frame.cpp:30-37
    int src_w = 0, src_h = 0, levels = 0, culls = 0;
    int w[DVO_MAX_LEVELS] = {0}, h[DVO_MAX_LEVELS] = {0};
    float K9[DVO_MAX_LEVELS][9];
    Intr k[DVO_MAX_LEVELS];
    size_t px_total = 0;  // sum over levels of w*h
    int top() const { return levels - 1; }
};
int make_geometry(const float K[9], int w, int h, int levels, int culls, Geometry& g);
// The per-level Intr make_geometry derives from K for the pyramid shape of g (the same operations: the same bits), and optionally
// the culled per-level K9 it derives them from
void level_intrinsics(const float K[9], const Geometry& g, Intr out[DVO_MAX_LEVELS], float (*K9_out)[9] = nullptr);
// Per-sequence intrinsics tables K[n][9] (dvo_batch_set_intrinsics, dvo_batch_create_mono_cameras): every entry finite, fx > 0 and
// fy > 0.  Otherwise DVO_ERR_BAD_ARGUMENT, with `who` and the index of the first bad sequence in the error message.
int check_intrinsics(const char* who, const float* K, size_t n);

struct FrameSet {  // n_seq frames: gray/depth/sigma pyramids, level l stored as [n_seq][h_l][w_l]
    Geometry g;
    int n_seq = 0;
    DevBuf arena;
    float* gray[DVO_MAX_LEVELS] = {nullptr};
    float* depth[DVO_MAX_LEVELS] = {nullptr};
    float* sigma[DVO_MAX_LEVELS] = {nullptr};
    // Per-pixel constant of a REFERENCE frame, derived once per frame instead of once per GN iteration:
    // wgt = step(level) / clamp(sigma) (optimize.cpp:83-84).  Same float operations, hoisted out of the iteration loop.
    float* wgt[DVO_MAX_LEVELS] = {nullptr};
    // Frames that came through the raw sensor conversion without a stored sigma pyramid carry sigma = 0.1 where depth > 0 and 1.0
    // elsewhere (transform.cpp:75): a pixel can only contribute with depth >= min_depth > 0, so its weight is the one constant
    // wgt_valid[level] and the wgt maps are neither written nor read (allow_const_weight: min_depth > 0).
    bool allow_const_weight = false, sigma_by_validity = false;
    float wgt_valid[DVO_MAX_LEVELS] = {0};
    float step[DVO_MAX_LEVELS] = {0};
    float sigma_min = 0.01f, sigma_max = 0.5f;
    int alloc(const Geometry& geo, int n, const dvo_config& cfg, void* mem = nullptr);   // mem: caller-owned block of arena_bytes()
    static size_t arena_bytes(const Geometry& geo, int n) { return 4 * geo.px_total * (size_t)n * sizeof(float); }
};

// Builds pyramids of (gray, depth, sigma) device inputs [n_seq][src_h][src_w]; depth/sigma may be null.
// keep_sigma = false: the sigma pyramid is only folded into `wgt`, not stored (frame-to-frame tracking never reads it again)
// seq_action / copy_from (Batch plan): the sequences whose effective action is DVO_SEQ_SKIP read no input and take copy_from's values
// ran (optional, here and below): the kernel the launcher chose (dvo_op_pyramid_frames)
void build_pyramid(FrameSet& fs, const float* gray_dev, const float* depth_dev, const float* sigma_dev, hipStream_t s, bool keep_sigma = true,
                   bool rows_decimated = false, const uint8_t* seq_action = nullptr, const FrameSet* copy_from = nullptr,
                   PyramidKernel* ran = nullptr);
// One frame of every sequence as handed over by the caller: float maps (gray [+ depth + sigma]) or raw sensor frames
// (u8 gray / RGB / RGBA [+ u16 depth], converted while the pyramid is built: loader.cpp:55-60,137-147, transform.cpp:60-76).
struct FrameInput {
    const float* gray = nullptr; const float* depth = nullptr; const float* sigma = nullptr;
    const uint8_t* rgb = nullptr; int channels = 0; const uint16_t* depth16 = nullptr; float depth_scale = 1.0f / 5000.0f;
    bool rows_decimated = false;  // the buffers hold only the rows the pyramid keeps (every 2^culls-th), see upload_rows
    // frames with lens undistortion (Undistortion::apply): k_pyramid_remap (mono: gray only) or k_pyramid_remap_depth (sensor depth)
    // gathers each kept pixel through its camera's table.  Whole frames (rows_decimated = false).
    const int* remap = nullptr;       // [n_cam][th][tw] source indices
    const int* remap_cam = nullptr;   // [n_seq] camera of each sequence
    // raw mono frames with a photometric calibration (Photometry::apply): the k_pyramid*_photo kernels.  Rows may be decimated
    // (the gain table is top-level sized) unless the frames are undistorted too.
    PhotoArgs photo{};
    // sensor-depth frames of a batch with dvo_batch_set_pyramid_filter: the gray pyramid is low-pass filtered before each halving
    // (k_pyramid_filter_top / _down).  Whole frames, no remap, never the split build.
    int filter = DVO_PYRAMID_FILTER_NONE;
    bool raw() const { return rgb != nullptr; }
    const void* key0() const { return raw() ? (const void*)rgb : (const void*)gray; }
    const void* key1() const { return raw() ? (const void*)depth16 : (const void*)depth; }
    bool has_depth() const { return raw() ? depth16 != nullptr : (depth != nullptr && sigma != nullptr); }
};
// The split build of a big batch's plain raw frames: the gray maps below the top level are built on `s`, where the
// tracker needs them first; the top-level gray and every depth level on `side`, which waits for `fork` (recorded on `s`, so every
// earlier launch that may still read the set is done) and records `done`.  Whoever reads what the side stream writes waits for `done`.
struct PyramidSplit {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, done = nullptr;
    hipError_t err = hipSuccess;   // of the event calls
};
// Returns true when the build was split (only with `split`, and only where pyramid_can_split allows it: a plan, a remap, float maps
// or an unusual alignment take the single kernel on `s`).
bool build_pyramid(FrameSet& fs, const FrameInput& in, hipStream_t s, bool keep_sigma = true, const uint8_t* seq_action = nullptr,
                   const FrameSet* copy_from = nullptr, PyramidSplit* split = nullptr, PyramidKernel* ran = nullptr);
// the sigma_by_validity a build of `in` into `fs` with keep_sigma = false would leave (the weight storage of the frame set)
inline bool weights_by_validity(const FrameSet& fs, const FrameInput& in) { return in.raw() && in.depth16 != nullptr && fs.allow_const_weight; }
// Host -> device copy of n_img images (raw or float; rows of row_bytes bytes).  With culls > 0 and decimate set only every
// 2^culls-th row of each image is transferred (one strided DMA): the pyramid never reads the others (Convert::cullImage keeps
// pixels whose coordinates are multiples of 2^culls), so 1 - 2^-culls of the PCIe traffic carries nothing.  Returns the bytes
// the device buffer holds through *stored.
int upload_rows(void* dst, const void* src, size_t row_bytes, int img_rows, size_t n_img, int culls, bool decimate, hipStream_t s,
                    size_t* stored);
inline bool can_decimate_rows(const Geometry& g) { return g.culls > 0 && (g.src_h % (1 << g.culls)) == 0; }
// Frame::updateDepthSigma / updateDepth (frame.cpp:39-61): re-decimate from a top-level map (may alias the top level)
void redecimate(FrameSet& fs, const float* depth_top, const float* sigma_top, hipStream_t s);

// Lens undistortion fused into the mono pyramid (dvo_batch_set_distortion, dvo_vo_set_distortion): Loader::getNormalizedUndistortedImages
// (loader.cpp:15-42) = dvo_op_undistort(frame, K_s, D_s) with each sequence's full-resolution creation K, applied to every frame before
// the pyramid.  The cameras are deduplicated by the bits of (fx, fy, cx, cy, D); k_undistort_map writes one table per camera, once.
struct Undistortion {
    std::vector<float> D;   // [n_seq][5] as set; empty: no undistortion (the handle runs exactly the kernels it runs without)
    DevBuf dev;             // [n_seq] int camera index (padded to 16 bytes), then [n_cam][th][tw] int tables
    int n_cam = 0;
    std::vector<int> cam_of;   // [n_seq] the camera index of each sequence, as on the device (Photometry pairs it with the calibration)
    const int* cam() const { return dev.as<int>(); }
    const int* table(int n_seq) const { return dev.as<int>() + (((size_t)n_seq + 3) & ~(size_t)3); }
    bool enabled() const { return !D.empty(); }
    // D: [5] (per_sequence = false) or [n_seq][5], nullptr clears; K_full: [n_seq][9], or [1][9] for every sequence (per_camera = false).
    // A non-finite coefficient: DVO_ERR_BAD_ARGUMENT naming `who` and the first bad sequence, nothing changed.
    int set(const char* who, const float* Dh, bool per_sequence, int n_seq, const float* K_full, bool per_camera, const Geometry& g, hipStream_t s);
    void apply(FrameInput& in, int n_seq) const
    {
        if (!enabled()) return;
        in.remap = table(n_seq); in.remap_cam = cam();   // (the caller uploads whole frames: rows_decimated = false)
    }
};

// Photometric calibration fused into the mono pyramid (dvo_batch_set_photometric, dvo_vo_set_photometric): n_cal
// inverse-response tables and vignette maps, one of them per sequence.  k_photometric_map writes one table of gains (1 / vignette at
// each kept pixel's source) per distinct (calibration, undistortion camera) pair of integers, once: at set, and again when D is set
// after it (the source of a kept pixel is then the remap's).  The per-frame kernels read response[cal][g8] * gain[pair][y][x].
struct Photometry {
    int n_cal = 0;                 // 0: none (the handle runs exactly the kernels it runs without)
    int n_pair = 0;
    std::vector<float> response;   // [n_cal][256] as used (a NULL response: k_ingest's scale, filled in)
    std::vector<float> vignette;   // [n_cal][src_h][src_w] as set; empty: 1
    std::vector<int> seq_cal;      // [n_seq]
    std::vector<int> seq_pair;     // [n_seq]
    DevBuf resp_dev, idx_dev, gain_dev;   // [n_cal][256]; [n_seq] cal then [n_seq] pair (each padded to 16 bytes); [n_pair][th][tw]
    bool enabled() const { return n_cal > 0; }
    // n == 0 clears.  Errors (DVO_ERR_BAD_ARGUMENT naming `who` and the first bad calibration / sequence) leave everything as it was.
    int set(const char* who, int n, const float* resp, const float* vign, const int* cal_of_seq, int n_seq, const Geometry& g,
            const Undistortion& und, hipStream_t s);
    int rebuild(int n_seq, const Geometry& g, const Undistortion& und, hipStream_t s);   // the gain tables from what is set now
    void clear()
    {
        n_cal = n_pair = 0;
        response.clear(); vignette.clear(); seq_cal.clear(); seq_pair.clear();
        resp_dev.release(); idx_dev.release(); gain_dev.release();
    }
    void apply(FrameInput& in, int n_seq) const
    {
        if (!enabled()) return;
        in.photo.response = resp_dev.as<float>(); in.photo.gain = gain_dev.as<float>();
        in.photo.seq_cal = idx_dev.as<int>(); in.photo.seq_pair = idx_dev.as<int>() + (((size_t)n_seq + 3) & ~(size_t)3);
    }
};

// The per-sequence actions of one Batch push, resolved on the device by k_plan (Batch::launch_plan)
struct TrackPlan {
    const uint8_t* action = nullptr;   // [n_seq] effective action: only DVO_SEQ_TRACK sequences are evaluated
    const int* lists = nullptr;        // n_sub lists ([0] = count, [4..] = local ids) of those sequences, n_seq + 4 ints apart
    volatile int* ready = nullptr;     // adaptive schedule: mapped host word, (tracked sequences + 1) once k_plan has run; nullptr: none
    const Intr* seq_k = nullptr;       // per-sequence intrinsics [level][n_seq] (dvo_batch_set_intrinsics); nullptr: Geometry::k
};

// Per-sequence start pose of a batch (dvo_batch_set_pose_guess_mode).  Allocated by the first mode set; from then on the
// seed kernel runs at every push, folding each push into the history even while the mode is NONE.  A batch that never sets a mode
// runs exactly the launches it ran before.
struct PoseGuess {
    int mode = DVO_GUESS_NONE;
    int n_seq = 0;
    DevBuf dev;                                // rows [n][6], start [n][6], hist [n][12] (float), then prev_eff [n], hist_n [n] (u8)
    HostRows given;                            // the rows of the next push (GIVEN); given.dev views rows()
    bool on() const { return dev.p != nullptr; }
    float* rows() const { return dev.as<float>(); }
    float* start() const { return dev.as<float>() + (size_t)n_seq * 6; }
    float* hist() const { return dev.as<float>() + (size_t)n_seq * 12; }
    uint8_t* prev_eff() const { return reinterpret_cast<uint8_t*>(dev.as<float>() + (size_t)n_seq * 24); }
    uint8_t* hist_n() const { return prev_eff() + n_seq; }
    // mode: the history starts from the last push: prev_eff_dev (its effective actions, device) or every sequence prev_all (0xff: none)
    int set_mode(int m, int n, hipStream_t s, const uint8_t* prev_eff_dev, int prev_all);
    PoseSeedArgs args(SeqState* state, const uint8_t* eff, int all_eff, const float* last_xi, const MonoSeq* meta) const;
    int last_start(float* out, hipStream_t s) const;
    void release(hipStream_t s) { given.release(s); }   // (PinnedPair's release order)
};

// Per-sequence tracking quality of a batch (dvo_batch_set_track_quality).  Allocated by the first enable; while on,
// Tracker::quality points at `rec`.  A read launches k_track_quality on the records of the last push / call.
struct Tracker;
struct TrackQuality {
    bool on = false;      // records are kept from the next push / call on
    bool ready = false;   // the last push / call kept them
    DevBuf rec, stage;    // [n_seq] dvo_gn_result; [n_seq] dvo_track_quality (staging of the host read)
    int set(bool enable, Tracker& trk, hipStream_t s);
    // status: the push's [n_seq] device status, or nullptr with every sequence `all_status`; out: device memory
    int launch(const Tracker& trk, const int* status, int all_status, dvo_track_quality* out, hipStream_t s) const;
    int read_host(const Tracker& trk, const int* status, int all_status, dvo_track_quality* out, hipStream_t s);
};

// What every opt-in term of batched tracking keeps (robust weights with any of their scales, affine brightness, the geometric term,
// step control): whether it is on, and the per-sequence record of the last push / call, which is all zeros for a
// push that tracked nothing.
struct OptInTerm {
    bool on = false;        // the next push / call runs with the term
    bool ready = false;     // the last push / call did
    bool tracked = false;   // ... and reached Tracker::track (else: nothing tracked, every record in `last` is zero)
    DevBuf last;            // [n_seq] records of the last push / call (the term says what a record is)
    void end_push(hipStream_t s)   // after every push / call of the owner, whether it tracked or not
    {
        if (on && !tracked) (void)hipMemsetAsync(last.p, 0, last.bytes, s);   // nothing tracked at this push
        ready = on;
        tracked = false;
    }
};

// Which terms combine.  A batch's state is the set of terms that are on (Term, dvo_kernels.h).  Each setter's "on" call
// is refused while one of the terms of its row of the table is on (Tracker::refusal); turning a term off never consults the table.
enum class TermSetter { RobustWeights, RobustMedian, AffineBrightness, Geometric, GeometricAffine, StepControl };
struct TermName { unsigned term; const char* is_on; const char* setter; };   // how a refusal names a term that is on

// Robust residual weights of a batch (dvo_batch_set_robust_weights).  Allocated by the first enable.  While on, the
// tracker runs the weighted plan (Tracker::lv_rw): k_track_gn_rw + k_gn_solve_rw pairs on every level.
struct RobustWeights : OptInTerm {
    int kind = DVO_ROBUST_NONE, mode = DVO_ROBUST_SCALE_ADAPTIVE;
    float param = 0.0f, floor2 = 0.0f;   // floor2 = scale_floor * scale_floor, once, in float
    DevBuf table;                        // [n_seq] RobustEntry.  last: [n_seq] float s2 of the last iteration
    HostRows scales;                     // GIVEN: [n_seq] float s; none: plain
    // The median scale (mode DVO_ROBUST_SCALE_MEDIAN: dvo_batch_set_robust_median), allocated by its first enable:
    // the pairs are k_track_gn_md + k_gn_solve_md, and the first iteration of the coarsest level follows a priming pair.
    DevBuf hist, hist_last;              // [n_seq][256] counts of the launch in flight; of each sequence's last evaluated iteration
    DevBuf mlog, prime_mn;               // [n_seq][levels][log_its][3] (s2 bits, m, n); [n_seq][2] the priming pair's (m, n)
    int log_its = 0;                     // iterations per level of the robust log
    bool median_ready = false;           // the last push / call ran with the median scale (its log and histogram can be read)
    bool median() const { return on && mode == DVO_ROBUST_SCALE_MEDIAN; }
    void end_push(hipStream_t s)         // OptInTerm's, and the median scale's own records
    {
        if (median() && !tracked) {   // nothing tracked at this push: no histogram and no priming record either
            (void)hipMemsetAsync(hist_last.p, 0, hist_last.bytes, s);
            (void)hipMemsetAsync(prime_mn.p, 0, prime_mn.bytes, s);
        }
        median_ready = median();
        OptInTerm::end_push(s);
    }
    void release(hipStream_t s) { scales.release(s); }   // (PinnedPair's release order)
};

// Affine brightness compensation of a batch (dvo_batch_set_affine_brightness).  Allocated by the first enable.  While on,
// the tracker runs the plan of launch pairs (Tracker::lv_rw): k_track_gn_ab + k_gn_solve_ab on every level, with or without robust weights.
struct AffineBrightness : OptInTerm {
    int mode = DVO_AFFINE_OFF;
    int min_pixels = 0;
    float min_contrast = 0.0f, gain_min = 0.0f, gain_max = 0.0f;
    int log_its = 0;                      // iterations per level of the affine log
    DevBuf table, prime;                  // [n_seq] AffineEntry; [n_seq][2] priming entry.  last: [n_seq][2] last used entry
    DevBuf moments, log;                  // [n_seq][part_rows][8] partial rows; [n_seq][levels][log_its][2]
    HostRows rows;                        // GIVEN: [n_seq][2] (a, b); none: (1, 0)
    void release(hipStream_t s) { rows.release(s); }   // (PinnedPair's release order)
};

// The geometric (depth) term of a sensor-depth batch (dvo_batch_set_geometric).  Allocated by the first enable.  While
// on, the tracker runs the plan of launch pairs (Tracker::lv_rw): k_track_gn_z + k_gn_solve_z on every level, on the tracked frame's
// own depth and weight maps.  With affine brightness on too (dvo_batch_set_geometric_affine) the pairs are
// k_track_gn_zab + k_gn_solve_zab, on the same maps.
struct GeometricTerm : OptInTerm {
    float weight = 0.0f, max_diff = 0.0f;
    int log_its = 0;        // iterations per level of the geometric log
    DevBuf log;             // [n_seq][levels][log_its][2] (n_geo, S29).  last: [n_seq][4] (n_geo, mean_sq, tracked, 0)
};

// Step control of a batch: damped Gauss-Newton with step acceptance (dvo_batch_set_step_control).  Allocated by the
// first enable.  While on, the tracker runs the plan of launch pairs (Tracker::lv_rw): the plain k_track_gn + k_gn_solve_lm on every
// level.  The tables are offset by the sub-batch's first sequence, like RobustEntry.
struct StepControl : OptInTerm {
    dvo_lm_config cfg{};
    int log_its = 0;        // iterations per level of the step-control log
    DevBuf table, log;      // [n_seq] dvo_lm_entry; [n_seq][levels][log_its][2] (lambda bits, decision).  last: [n_seq] dvo_lm_record
};

// How one pyramid level is launched.  Decided once by Tracker::init and fixed from then on: Tracker::gn_args and Tracker::solve_args
// copy the geometry from here into every argument block, and the launchers take the kernel instance from here.
struct LevelPlan {
    int ppt = 0, group = 0;          // pixels per thread and gather group: the kernel instance
    int nblk = 0;                    // tiles (= partial rows) per sequence
    GnTiling tiling;                 // the tiles of k_track_gn and of every kernel that shares them (margin == 0; else the default)
    int tiles_x = 0, tiles_y = 0;    // the tiles of k_track_gn_tile (margin > 0, gn_tile_geometry; else 0)
    // The level's launch form, a DVO_PLAN_* value of include/dvo.h: PAIRS = k_track_gn + k_gn_solve per iteration,
    // ITERATION = one k_track_gn_fused per iteration (small handles: see dvo_kernels.hip), LEVEL = ONE k_track_level launch (all
    // iterations on the device), LDS_PATCH = k_track_gn_tile + k_gn_solve per iteration.  Everything that launches reads it from here.
    int schedule = DVO_PLAN_PAIRS;
    int margin = 0;                  // the LDS-staged reference patch's margin: 0 unless schedule == DVO_PLAN_LDS_PATCH
};

// Which partial rows a solve sums (SolveArgs::blk_first / blk_count) and what it adds to the profile counter (SolveArgs::level_pixels)
enum class SolveRows {
    All,        // every row, w * h pixels: k_track_gn_tile's solves, k_track_level
    Live,       // the level's live tiles, w * h pixels: the solves that feed no profile counter (k_track_gn_fused, dvo_op_gn_step)
    LivePair,   // the level's live tiles and the pixels they cover: the k_gn_solve after a k_track_gn
};

struct TrackCall;   // one track() call's state (dvo_engine.cpp)

struct Tracker {  // Track::Tracker for n_seq sequences at once
    Geometry g;
    int n_seq = 0;
    dvo_config cfg;
    DevBuf state, partials, log, counters, xi_out, T_out;
    // partial rows reserved per sequence: the largest nblk of any level.  A sub-batch's rows start at q0 * part_rows on every level,
    // so sub-batches on concurrent streams, which reach the levels at different times, never share a row
    size_t part_rows = 0;
    // Two active-sequence lists per sub-batch ([0] = count, [4..] = ids local to the sub-batch), written by k_gn_solve,
    // read by the next k_track_gn.
    DevBuf work;
    int* work_list(int sub, int i) const { return work.as<int>() + (size_t)(2 * sub + (i & 1)) * (size_t)(n_seq + 4); }
    // Sub-batches: the sequences are split into n_sub contiguous groups whose launch chains (k_track_gn -> k_gn_solve ->
    // ...) run on concurrent HIP streams, so one group's latency-bound solve / launch gaps are covered by another
    // group's work.  Group 0 uses the caller's stream; fork/join events order the groups against it.
    int n_sub = 1;
    std::vector<hipStream_t> sub_streams;  // n_sub - 1 library-owned streams
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    int sub_first(int k) const { return (int)(((long long)n_seq * k) / n_sub); }
    LevelPlan lv[DVO_MAX_LEVELS];
    // Both plans are decided by init: lv_plain is what the configuration asks for, lv_rw the weighted plan (launch pairs of the
    // global-gather kernel on every level, whatever track_fused_tiles, gn_use_lds_patch, track_single_launch and the batch size say).
    // lv is whichever is in force (use_plan, called by set_term: any opt-in term runs the weighted plan).  What init decided from
    // the configuration alone -- n_sub, adaptive, persist_ok -- stays as it is under either plan.
    LevelPlan lv_plain[DVO_MAX_LEVELS], lv_rw[DVO_MAX_LEVELS];
    void use_plan();
    // the rows a level's solve sums behind its k_track_gn (`live`: Live or LivePair) or k_track_gn_tile (All) launch
    SolveRows pair_rows(int level, SolveRows live) const;
    int log_iterations() const;   // iterations per level an opt-in term's log holds (fixed by the term's first enable)
    // One iteration's launch pair of the terms that are on: each fills the block of every such term and makes one call, and the
    // kernel file's table picks the pair (launch_track_gn_terms / launch_gn_solve_terms); with nothing on, launch_gn
    // and launch_gn_solve.  `ga` / `sa` view `count` sequences (their SeqState offset is every table's).  DVO_ERR_HIP, and nothing
    // launched, for a set of terms without a kernel pair (an internal error: refusal lets none through).
    //   ref_z: the reference's depth of the level (whole batch, like GnArgs::ref_gray before gn_view; the geometric term only)
    //   prime: the priming pair of affine ESTIMATE mode or of the median robust scale
    struct SolveTerm {   // what a solve's caller chooses, value-initialised; the outputs are the one-evaluation ops' (device memory)
        bool adaptive_scale;      // the solve writes the next RobustEntry from this iteration's residual
        bool prime;               // the priming pair
        bool estimate_once;       // the affine solve writes the next entry whatever the mode (dvo_op_gn_step_affine)
        double* geo_sums;         // the geometric term: 2 doubles (n_geo, S29)
        double* affine_moments;   // affine brightness: DVO_AFFINE_MOMENTS doubles
        int* step_mn;             // the median scale: 2 ints (m, n)
    };
    int launch_gn_term(const GnArgs& ga, int level, int count, hipStream_t s, int grid_seqs = 0, const float* ref_z = nullptr,
                       bool prime = false) const;
    int launch_solve_term(const SolveArgs& sa, int count, hipStream_t s, const SolveTerm& t) const;
    // The terms' begin of a call, before the fork (every sub-batch reads its part of the tables): the weight table (k_robust_begin),
    // the median scale's counts, the brightness table (k_affine_begin), the geometric records cleared ("not tracked" until a solve
    // says otherwise), step control's lambda0 and empty records.  once: the one-evaluation ops' given s2 and (a, b) of every sequence.
    struct GivenOnce { float s2, a, b; };
    int begin_terms(hipStream_t s, const GivenOnce* once = nullptr);
    void end_terms(hipStream_t s);          // after every push / call of the owner, whether it tracked or not (every opt-in term)
    // The setters (configurations validated by the caller; nullptr or the term's OFF / NONE mode: off).  Every one goes through
    // set_term: an "on" call is refused with DVO_ERR_BAD_ARGUMENT, naming `who`, the offending term and its setter, while a term it
    // does not combine with is on (refusal: the table) and then changes nothing; the plan follows what is on.
    unsigned terms_on() const;
    static const TermName* refusal(unsigned on, TermSetter want);   // the term that refuses `want`, nullptr: allowed
    GeometricTerm geo;
    int set_geometric(const char* who, const dvo_geometric_config* c, hipStream_t s);
    int set_geometric_affine(const char* who, const dvo_geometric_config* gc, const dvo_affine_config* ac, hipStream_t s);   // both on
    int last_geometric(dvo_geometric_record* rec, hipStream_t s) const;
    int last_geometric_log(int seq, dvo_geometric_log* out, hipStream_t s) const;
    StepControl lm;
    int set_step_control(const char* who, const dvo_lm_config* c, hipStream_t s);
    int last_step_control(dvo_lm_record* rec, hipStream_t s) const;
    int last_step_control_log(int seq, dvo_lm_log* out, hipStream_t s) const;
    AffineBrightness aff;
    int set_affine(const char* who, const dvo_affine_config* c, hipStream_t s);
    int last_affine(float* ab, hipStream_t s) const;
    int last_affine_log(int seq, dvo_affine_log* out, hipStream_t s) const;
    RobustWeights rob;
    int set_robust(const char* who, const dvo_robust_config* c, hipStream_t s);   // (the median scale is c->scale_mode)
    int last_robust_scales(float* s2, hipStream_t s) const;
    int last_robust_log(int seq, dvo_robust_log* out, hipStream_t s) const;          // the median scale
    int last_robust_histogram(int seq, uint32_t* counts, hipStream_t s) const;
    DevBuf ticket, freport;      // k_track_gn_fused: arrival tickets [n_seq]; (reported, active) per (set, level, iteration)
    // Adaptive schedule: progress words in mapped host memory, one per (level, iteration), two sets used alternately.
    // k_gn_solve's workgroup 0 stores (active sequences + 1); the host reads them to stay ~2 iterations ahead of the GPU and
    // to stop enqueuing a level once a launch reported zero active sequences (its remaining launches would be empty).
    int* h_progress = nullptr;   // host view
    int* d_progress = nullptr;   // device view of the same memory
    int progress_set = 0;
    bool adaptive = false;
    SeqState* h_state = nullptr;  // pinned host mirror of `state` for the small-batch convergence poll
    // k_track_gn_tile (the level's schedule is DVO_PLAN_LDS_PATCH) or k_track_gn (global gathers: every other schedule)
    void launch_gn(const GnArgs& a, int level, int count, hipStream_t s, int grid_seqs = 0) const;  // `a` views `count` sequences
    // per-sequence intrinsics [level][n_seq] of a per-camera mono batch (dvo_batch_create_mono_cameras), used when track() has no
    // plan (a plan brings its own, TrackPlan::seq_k); nullptr: Geometry::k.  Never set together with prefer_persist.
    const Intr* cam_k = nullptr;
    // start pose of the next track() (a batch's dvo_batch_set_pose_guess_mode): k_seed_pose, or with seed_mono k_mono_seed, runs after
    // k_track_begin (or the caller's k_plan) and before the sub-batch fork; nullptr: every sequence starts from zero.  Never with persist.
    const PoseSeedArgs* seed = nullptr;
    bool seed_mono = false;
    // the split pyramid build of the next track()'s obj (PyramidSplit::done): its top level and its depth maps are still being written
    // on another stream.  track() waits for it on every stream that launches the top level, before the first such launch, and on `s`
    // before it returns whatever the schedule did; nullptr: obj is complete in stream order.
    hipEvent_t top_ready = nullptr;
    // a batch's quality records (dvo_batch_set_track_quality): while set, every solve of the finest level stores its sums here
    // (SolveArgs::result, [n_seq]), so each sequence's last one remains; nullptr: no record (the plain path's kernel arguments)
    dvo_gn_result* quality = nullptr;
    // One launch per track() call (k_track_persist) for a single sequence whose result is handed over through h_result: eligible
    // when every level fits the kernel's wide reduction and shares one tile size; `persist_failed` = a launch gave up waiting
    // (GPU oversubscribed): the handle then stays on the launch-per-iteration schedule.
    bool prefer_persist = false;   // set before init() by the owner whose results go through enable_host_result() (VisualOdometry's sensor-depth tracker)
    bool persist_ok = false, persist_failed = false, persist_used = false;
    // this track() call runs as k_track_persist (an owner arms mono_tail by it, with plan = nullptr: what it then passes to track())
    bool persist_call(const TrackPlan* plan = nullptr) const { return persist_ok && !persist_failed && h_result && !plan && !cam_k && !seed; }
    int persist_grid = 0, persist_spin_limit = 1 << 18;
    bool persist_timeline = false;   // DVO_PERSIST_TIMELINE is set, to the worker whose stamps are kept beside the solver's
    int persist_dbg_worker = 0;
    DevBuf persist_ctl, persist_dbg;
    int read_persist_timeline(long long* out);
    const FrameSet* last_obj = nullptr; const FrameSet* last_ref = nullptr;
    // Result hand-over for a handle that returns one pose per call (dvo_vo): k_export_poses also writes xi, T and a tag into
    // fine-grained mapped host memory, and wait_host_result() polls the tag -- no device-to-host copy, no stream synchronisation.
    float* h_result = nullptr;   // host view: [0..5] xi, [6..21] T, [22] tag (int), [23] tag of a persistent launch that gave up
    float* d_result = nullptr;   // device view of the same memory
    int result_tag = 0;
    PersistMono mono_tail{};       // armed by a mono dvo_vo handle before track(): k_track_persist also does k_mono_decide's work
    int persist_ppt = 0;           // pixels per thread of the one-launch schedule: 0 = 4, > 0 = that many, < 0 = what the other schedules pick
    int enable_host_result();
    int wait_host_result(hipStream_t s, float xi[6], float T[16]);   // of the last track() call
    // profiling (cfg.profile)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    double prof_ms = 0;
    uint64_t prof_launches = 0;
    ~Tracker();
    int init(const Geometry& geo, int n, const dvo_config& c);
    GnParams level_params(int level) const;
    // The arguments of a level's Gauss-Newton launches for all n_seq sequences, tile geometry included (lv[level]); from the level's
    // five maps, or from the frame sets that hold them
    GnArgs gn_args(const float* obj_gray, const float* ref_gray, const float* ref_depth, const float* ref_wgt, float wgt_const, int level,
                   uint8_t* mask, int ignore_active) const;
    GnArgs gn_args(const FrameSet& obj, const FrameSet& ref, int level, uint8_t* mask, int ignore_active) const;
    // `all` as seen by the sub-batch that starts at sequence q0: its part of every per-sequence array
    GnArgs gn_view(const GnArgs& all, int level, int q0, const TrackPlan* plan, const Intr* seq_k) const;
    // what every solve of a level shares, for the sequences from q0 on, summing `rows`; each schedule adds its own fields
    SolveArgs solve_args(int level, int q0, int ignore_active, SolveRows rows) const;
    int next_result_tag();   // the tag of this call's result (never 0)
    // the whole call in one k_track_persist launch; persist_used stays false: there is no instance, the caller runs the other schedules
    int track_persist(const FrameSet& obj, const FrameSet& ref, hipStream_t s);
    // Tracker::track (tracker.cpp:22-85): enqueue the whole coarse-to-fine loop; poses land in xi_out / T_out
    // With a plan (Batch): k_plan has done k_track_begin's work, and a level's first iteration runs the plan's sequences, not all
    int track(const FrameSet& obj, const FrameSet& ref, hipStream_t s, const TrackPlan* plan = nullptr);
    int collect_profile(hipStream_t s);
private:
    // The pieces of track(), around one call's TrackCall: what is queued ahead of the levels, the three launch forms
    // of one sub-batch (switch (lv[level].schedule)), and the host's two pacing mechanisms ahead of and behind an iteration
    int track_prologue(TrackCall& c);
    int wait_top(TrackCall& c, int streams);
    void queue_level(const GnArgs& ga, int level, int q0, int nq, hipStream_t sk);
    int queue_iteration(const TrackCall& c, const GnArgs& ga, int level, int it, int q0, int nq, hipStream_t sk);
    int queue_pair(const TrackCall& c, GnArgs ga, int level, int it, int k, int q0, int nq, hipStream_t sk, int active_ub, const float* ref_z);
    int wait_ahead(const TrackCall& c, int level, int it);
    int poll_active(const TrackCall& c, int level, int it, bool* go);
    // the one place every setter goes through: the table (an "on" call only), the term's own `apply`, the plan of what is on now
    template <class Apply> int set_term(const char* who, TermSetter want, bool enable, Apply&& apply);
    int apply_robust(const dvo_robust_config* c, hipStream_t s);
    int apply_affine(const dvo_affine_config* c, hipStream_t s);
    int apply_geometric(const dvo_geometric_config* c, hipStream_t s);
    int apply_step_control(const dvo_lm_config* c, hipStream_t s);
    // The log of sequence `seq` at the last push / call: `words` values of W per logged iteration in `log_dev`
    // ([n_seq][levels][log_its][words]) and the term's record of the sequence, last_dev; `extra`: one more copy ahead of the one
    // synchronize (a priming record).  Zeroes *out but its struct_size, sets levels and, when tracked(record) says the sequence
    // tracked at that push, n_iter (clamped to log_its) and calls unpack(level, it, row) for every logged iteration.
    struct LogCopy { void* dst; const void* src; size_t bytes; };
    template <class W, class Last, class Log, class Tracked, class Unpack>
    int read_term_log(const W* log_dev, int words, int log_its, int seq, const Last* last_dev, Log* out, hipStream_t s, Tracked tracked,
                      Unpack unpack, LogCopy extra = {}, bool* did_track = nullptr) const;
    // the argument blocks of the opt-in terms' kernels for the sequences from q0 on (launch_gn_term, launch_solve_term)
    RobustSolve robust_solve_args(size_t q0, bool adaptive) const;
    MedianSolve median_solve_args(size_t q0, bool log, bool prime, int* step_mn) const;
    GeoGn geo_gn_args(size_t q0, int level, const float* ref_z) const;
    GeoSolve geo_solve_args(size_t q0, bool log, double* sums_out) const;
    AffineGn affine_gn_args(size_t q0, bool prime) const;
    AffineSolve affine_solve_args(size_t q0, bool log, bool prime, double* moments_out, bool estimate_once) const;
    LmSolve lm_solve_args(size_t q0, bool log) const;
};

struct Keyframe {  // System::Frame of one sequence, plus the age map and pose (frame.hpp:72-144)
    FrameSet fs;
    DevBuf age;    // top-level [h][w]
    DevBuf depth_alt;              // second top-level depth map: k_regularize_redecimate writes the regularized map beside the one it reads
    float* depth_spare = nullptr;  // whichever of the arena's top-level block and depth_alt fs.depth[top] does not point to
    float xi[6] = {0, 0, 0, 0, 0, 0}, rel_xi[6] = {0, 0, 0, 0, 0, 0};
    int id = -1, ref_id = -1;
    KeyframePool* pool = nullptr;  // where `block` (the memory of all three buffers) goes back to
    void* block = nullptr;
    int alloc(const Geometry& g, const dvo_config& cfg, KeyframePool* from = nullptr);
    ~Keyframe() { if (pool && block) pool->give(block); }
};

struct VisualOdometry {  // System::VisualOdometry, system.hpp:12-104
    float K[9];
    int w = 0, h = 0, device = 0;
    dvo_config cfg;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Geometry geoM, geoD;  // Frame(gray,K,3,2) (system.hpp:47) and Frame(g,d,s,K,4,1) (system.hpp:82)
    Tracker trkM, trkD;
    bool trkM_ready = false, trkD_ready = false;
    KeyframePool kf_pool;                              // (declared before the keyframes: destroyed after them)
    std::vector<std::unique_ptr<Keyframe>> hist;       // FrameHistory, oldest first
    std::unique_ptr<Keyframe> scratch;                 // the frame being processed (promoted on keyframe)
    std::unique_ptr<Keyframe> depth_ref, depth_cur;    // m_ref_frame of odometrizeUsingDepth
    DevBuf in_gray, in_depth, in_sigma;                // full-resolution staging
    DevBuf tmp_a, tmp_b, tmp_c, owner, ages, valid_dev;
    // Mapper state of this sequence on the device (the same kernels as the batched mono pipeline: k_mono_decide, k_age_table),
    // so that a dvo_vo handle and a sequence of a mono dvo_batch produce identical bits.
    DevBuf meta_dev, hist_xi_dev, gray_tab_dev;
    MonoSeq h_meta;
    void* h_pin = nullptr;   // pinned staging for the per-frame read-back (MonoSeq + track log)
    std::vector<float> init_depth, init_sigma;
    int latest_id = -1;                                // Frame::latest_id, frame.cpp:5
    int history_limit = 0;                             // 0 = keep every keyframe (the reference); N = keep the newest N
    int last_id = -1, last_valid_updates = 0;
    bool valid_updates_pending = false;                // last_valid_updates is stale: the count of the last map_update is still on the device
    int fetch_valid_updates();
    // device copies of FrameHistory's poses / gray pointers (k_age_table, k_depth_update): refreshed when the history changes

    int hist_table_n = -1;
    unsigned long long hist_version = 0, hist_table_version = ~0ull;   // hist_version: bumped wherever `hist` changes
    float last_xi[6] = {0}, last_rel[6] = {0};
    dvo_track_log last_log;
    Tracker* log_src = nullptr;                        // the tracker whose device log is newer than last_log (read back on demand only)
    int fetch_log();                                   // dvo_vo_last_track_log: the 15 KB per-iteration record is copied when asked for
    ~VisualOdometry();
    int init(const float K9[9], int width, int height, const dvo_config* c);
    int odometrize(const float* gray, float T_world[16], int* is_key, const uint8_t* raw = nullptr, int raw_channels = 0);
    int odometrize_depth(const float* gray, const float* depth, const float* sigma, float T_rel[16]);
    int odometrize_depth_raw(const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale, float T_rel[16]);
    int odometrize_depth_staged(float T_rel[16], const struct FrameInput* raw = nullptr,   // frame already staged on the device
                                const std::function<int()>* after_launch = nullptr);
    Undistortion und;      // dvo_vo_set_distortion: the mono frames (odometrize) are undistorted while their pyramid is built
    bool fed = false;      // a frame went through odometrize* or init_keyframe (dvo_vo_load does not count): D is fixed from then on
    int set_distortion(const float D[5]);
    Photometry pho;        // dvo_vo_set_photometric: the raw mono frames (odometrize) are calibrated while their pyramid is built
    int set_photometric(const float* resp, const float* vign);
    DevBuf raw_rgb, raw_depth;
    // the maps of one frame go up on separate streams: three strided copies queued on one stream run one after the other with
    // ~9 us between them (98 us from the end of one frame's tracking to the next pyramid, profiles/r03_single_hip_trace.txt)
    hipStream_t ustream[2] = {nullptr, nullptr};
    hipEvent_t uevent[3] = {nullptr, nullptr};
    int upload_streams();
    bool side_built = false;   // uevent[1] marks a depth / sigma pyramid built on the side stream (odometrize_depth)
    bool decimate_host_rows = getenv("DVO_UPLOAD_FULL_FRAMES") == nullptr;  // as HostStage::decimate_host_rows
    int init_keyframe(const float* gray, const float* depth, const float* sigma);
    int map_propagate(Keyframe& frame, const Keyframe& ref);
    int map_update(Keyframe& obj);
    int refresh_history_tables();
    int alloc_stage();
    bool stage_mono_rows = true, stage_raw_rows = true;   // frames reach the pyramid kernel through the staging block (DVO_MONO_STAGE / DVO_RAW_STAGE = 0: runtime copies)
    void* h_stage = nullptr;       // pinned, device-mapped staging of a mono frame's kept rows (k_pyramid reads it through d_stage)
    void* d_stage = nullptr;
    void* h_tables = nullptr;      // pinned staging of the history tables
    size_t h_tables_bytes = 0;
    bool age_table_done = false;   // this frame's age table came out of k_track_persist's tail
    int map_regularize(Keyframe& kf);
};

// The per-sequence action plan of a batch of either kind (dvo_batch_set_actions / dvo_batch_set_mono_actions): what
// k_plan reads and writes, the staging of host actions and the ready words of the adaptive schedule.  Allocated on first use; a batch
// that never sets actions runs the plain path.
struct SeqPlan {
    // has_ref: the sequence has something to track against (sensor depth: a reference frame; mono: a keyframe)
    DevBuf act_dev, has_ref, eff, status, lists, tally;
    PinnedPair act_stage;                       // pinned staging of host actions
    int* h_ready = nullptr;                     // mapped host words of TrackPlan::ready, one per parity
    int* d_ready = nullptr;
    const uint8_t* act_src = nullptr;           // actions of the next push / call (device memory)
    bool act_pending = false, act_used = false;
    int parity = 0;                             // which of the two list sets (and ready words) the next plan writes
    int alloc(int n_seq, int n_sub, bool has_ref_fill, hipStream_t s);   // on first use; later calls do nothing
    int set_actions(const uint8_t* actions, bool on_device, int n_seq, hipStream_t s);   // (after alloc, unless actions is null)
    // k_plan's arguments for this push / call, all but cam_changed; with track_follows under the adaptive schedule the ready word
    // of this parity is reset and handed to the kernel
    PlanArgs plan_args(const Tracker& trk, bool track_follows);
    TrackPlan track_plan(const Tracker& trk) const;   // (all but seq_k)
    void consumed();
    // the status of the last push / call; before any actions were used: every sequence STARTED (first_push) or TRACKED
    int status_of_last(int* out, bool out_on_device, int n_seq, bool first_push, hipStream_t s) const;
    void release(hipStream_t s);                // (PinnedPair's release order)
    ~SeqPlan() { release(nullptr); }

private:
    int* list_set(const Tracker& trk, int which) const { return lists.as<int>() + (size_t)which * trk.n_sub * (size_t)(trk.n_seq + 4); }
};

// Host input of a batch of either kind: two staging slots filled on a copy stream, so the H2D transfer of frame k+1 runs beside the
// tracking of frame k (PCIe is the bound of a host-fed batch: 0.92 MB per raw 640x480 frame).  Slot k & 1 is reused by push k + 2,
// whose copy waits until push k (pyramid build + tracking) is done with it.
struct HostStage {
    struct Slot { DevBuf buf[3]; hipEvent_t copied = nullptr, consumed = nullptr; bool used = false; } slot[2];
    hipStream_t cstream = nullptr;
    int n_push = 0, k = 0;   // frames taken; the slot of the frame being staged (begin)
    bool decimate_host_rows = getenv("DVO_UPLOAD_FULL_FRAMES") == nullptr;  // transfer only the rows the pyramid keeps
    // only the rows the pyramid keeps cross PCIe (the staging buffers are sized for whole frames) -- unless the frames are undistorted:
    // the remap reads any row, so whole frames go up (4x the bytes at cull 2)
    bool decimate(const Geometry& g, const Undistortion& und) const { return decimate_host_rows && can_decimate_rows(g) && !und.enabled(); }
    Slot& cur() { return slot[k]; }
    int begin();                              // the copy stream and events on first use; this frame's slot, once its last user is done
    int upload(int i, const void* src, size_t row_bytes, const Geometry& g, int n_seq, bool decimate);   // one map of every sequence -> buf[i]
    int end_copy(hipStream_t tracking, bool all_sources_pinned);   // the tracking stream waits for this frame's copies
    int consumed(hipStream_t tracking);       // everything queued on the tracking stream so far is this slot's last user
    void advance() { n_push++; }              // (its own call: the two batch kinds differ in when a refused frame counts)
    void release();                           // (PinnedPair's release order; the copy stream is its own)
    ~HostStage() { release(); }
};

// Keyframe maps as compacted world-frame point clouds (dvo_batch_export_points), shared by both batch kinds: each
// kind fills a Source (where its keyframes' planes, twists, flags and intrinsics live) and run() launches k_points_prep and
// launch_points on the handle's stream.  Allocated on first use; a batch that never exports runs the launches it always ran.
struct PointsExport {
    DevBuf table, seq_total, chunk_count, offsets;   // PointsSeq [n_seq]; uint32 [n_seq]; uint32 [n_seq][chunks of the top level]; uint32 [n_seq + 1]
    bool ready = false;                              // an export has been queued (dvo_batch_last_points)
    struct Source {
        const MonoSeq* meta = nullptr;
        const uint8_t* started = nullptr; int started_by_total = 0;   // PointsPrepArgs
        const int* is_key = nullptr;
        const float* depth = nullptr; const float* gray = nullptr; const float* sigma = nullptr; const float* age = nullptr;
        const uint8_t* counts = nullptr;
        const Intr* seq_k = nullptr; Intr k{};
        int w = 0, h = 0, top_w = 0, top_h = 0, n_seq = 0;
    };
    // cfg: validated, level and min_depth resolved (dvo_capi)
    int run(const Source& src, const dvo_points_config& cfg, uint32_t capacity, float* xyzg, uint32_t* src_idx, float* sigma_out,
            uint32_t* offsets_out, hipStream_t s);
};

struct Batch {  // n_seq independent sequences, frame-to-frame (or keyframe) tracking with sensor depth
    int n_seq = 0, device = 0;
    dvo_config cfg;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Geometry g;
    Tracker trk;
    // Three frame sets: the reference (cur), the frame being tracked against it, and one that the pyramid of a LATER frame can
    // be built into on a low-priority side stream while tracking runs (prefetch_device): k_pyramid is HBM bound, the tracker
    // mostly VALU / latency bound.
    FrameSet fs[3];
    int cur = -1;           // frame set of the newest tracked frame = reference of the next (-1: none yet)
    int prev = -1;          // its own reference (probes)
    // prefetched frame sets waiting for their push_device, oldest first.  In steady state two are outstanding at the moment
    // prefetch_device is called: "prefetch(k+1); push(k)" finds frame k (prefetched one step earlier) still waiting.
    int preq[2] = {-1, -1};
    int npre = 0;
    const void* pre_key[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipStream_t pstream = nullptr;
    hipEvent_t ev_last_track = nullptr, ev_built[3] = {nullptr, nullptr, nullptr};
    bool tracked_once = false;
    bool have_poses = false;
    // The split pyramid build of a plain push of raw frames: stage B runs on pstream beside the coarse-level launches.
    // Every push queues the wait for split.done on `stream` before it returns (Tracker::track before the first top-level launch, or
    // push itself when nothing tracks), so whatever follows on the stream -- copies, exports, the next push, destruction -- is ordered
    // after stage B.  DVO_PYRAMID_SPLIT: 0 = never, 1 = always, unset = batches of at least 1 024 sequences (below, a level is a
    // latency chain and a second launch only adds to it).
    PyramidSplit split;
    bool split_on = false;
    HostStage host;         // host input (push_host / push_raw_host): up to three maps per frame
    int push_host_frame(const void* p0, const void* p1, const void* p2, FrameInput in);
    ~Batch();
    int init(int n, const float K9[9], int w, int h, int levels, int culls, const dvo_config* c);
    int free_slot() const  // a frame set that is neither the reference nor waiting prefetched (-1: none)
    {
        for (int i = 0; i < 3; i++)
            if (i != cur && !(npre > 0 && preq[0] == i) && !(npre > 1 && preq[1] == i)) return i;
        return -1;
    }
    int prefetch(const FrameInput& in);
    int push(const FrameInput& in);
    // Per-sequence skip / restart (dvo_batch_set_actions).  Allocated on first use; a batch that never sets actions runs the plain path.
    SeqPlan plan;
    int n_push = 0;
    int alloc_plan() { return plan.alloc(n_seq, trk.n_sub, cur >= 0, stream); }   // (every sequence that a plain push gave a frame has a reference)
    int set_actions(const uint8_t* actions, bool on_device);
    int launch_plan(bool track_follows);
    int status_of_last(int* out, bool out_on_device);
    int check_actions_input(const FrameInput& in) const;
    // Per-sequence intrinsics (dvo_batch_set_intrinsics).  Allocated on first use; once set, every push runs the per-sequence path.
    float K_create[9] = {0};                    // the K of dvo_batch_create (set_intrinsics(NULL) goes back to it)
    std::vector<float> cam_K;                   // [n_seq][9] the table of the next push (creation K until set)
    std::vector<float> cam_K_used;              // [n_seq][9] the table of the last push (the camera-change rule compares the two)
    DevBuf cam_dev;                             // [level][n_seq] Intr, then [n_seq] camera-changed bytes of the next push
    PinnedPair cam_stage;                       // pinned staging of cam_dev
    bool cam_pending = false, cam_used = false;
    int set_intrinsics(const float* K);
    int stage_cameras(const float* K);          // the table of the next push + its camera-changed bytes (K: [n_seq][9], nullptr: creation K)
    // Lens undistortion of the sensor-depth frames (dvo_batch_set_sensor_distortion): k_pyramid_remap_depth gathers every kept pixel
    // through the table of the sequence's (current K, D).  A sequence's camera is (fx, fy, cx, cy, D or none): a change of D at a push
    // sets its camera-changed byte as a change of K does.
    Undistortion und;                           // D and the tables of the next push (built from cam_K)
    std::vector<float> und_D_used;              // [n_seq][5] the D of the last push (empty: none)
    bool und_pending = false;                   // und changed since the last push
    int set_sensor_distortion(const float* D, bool per_sequence);
    // The gray pyramid's low-pass filter (dvo_batch_set_pyramid_filter): fixed once a frame was pushed or prefetched.
    // While it is on every build takes launch_pyramid's filter branch on whole frames (host feeds upload every row) and is not split.
    int pyr_filter = DVO_PYRAMID_FILTER_NONE;
    int set_pyramid_filter(int filter);
    bool distortion_changed(size_t q) const
    {
        if (und.enabled() != !und_D_used.empty()) return true;
        return und.enabled() && memcmp(&und.D[q * 5], &und_D_used[q * 5], 5 * sizeof(float)) != 0;
    }
    const Intr* cam_table() const { return cam_used ? cam_dev.as<Intr>() : nullptr; }
    PoseGuess guess;                            // dvo_batch_set_pose_guess_mode / dvo_batch_set_pose_guess
    int set_guess_mode(int mode);
    // the seed of this push outside track() (a push that tracks nothing still folds into the history)
    void seed_untracked(const uint8_t* eff_dev, int all_eff);
    PoseSeedArgs guess_args(const uint8_t* eff_dev, int all_eff);   // (keyframe tracking: world twists and the keyframe twists, k_mono_seed)
    TrackQuality quality;                       // dvo_batch_set_track_quality
    const uint8_t* cam_changed() const { return reinterpret_cast<const uint8_t*>(cam_dev.as<Intr>() + (size_t)g.levels * n_seq); }
    // Keyframe tracking (dvo_batch_set_keyframe_tracking): every push runs the per-sequence path; the first push's frame
    // set (cur) is the keyframe set and is never rotated away, later frames are built into another set and tracked against it.  After
    // the tracking, k_kf_decide takes the mono rule (mono_decide_one) per sequence and k_promote copies the frames of the sequences
    // whose rule fired, and of the starts, over their keyframes.  Chosen before the first push; a batch that never sets it runs the
    // launches it always ran.
    bool kf_on = false;
    DevBuf kf_meta, xi_world, T_world, is_key, need_list;   // MonoSeq [n_seq]; [n_seq][6], [n_seq][16], [n_seq]; [4 + n_seq]
    int set_keyframe_tracking(int enable);
    int update_keyframes(int frame_set);                     // k_kf_decide, then k_promote from fs[frame_set] into fs[cur]
    // What keyframe fusion and keyframe carry both keep: the switch, the table their prep kernel fills and the records of the last push.
    struct KfStage {
        bool on = false;
        bool ready = false;      // the last push ran with it on (dvo_batch_last_keyframe_fusion / _carry)
        DevBuf table, rec;       // KfSeq [n_seq]; KfRecord [n_seq]
        int alloc(DevBuf& plane, size_t n_seq, size_t npix);   // the stage's uint8 [n_seq][npix] plane, its table and records: once
    };
    // Keyframe depth fusion (dvo_batch_set_keyframe_fusion): after the promotions of a push, k_kf_fuse_prep and k_kf_fuse
    // fold the tracked frame's top-level depth into the keyframes of the sequences that tracked without firing the rule, and clear the
    // counts of those that started or promoted.  Off (the default): update_keyframes launches what it always launched.
    struct KfFusion : KfStage {
        bool ran = false;        // some push ran with fusion on (dvo_batch_keyframe_fusion_counts)
        dvo_kf_fusion_config cfg = {DVO_KF_FUSION_OFF, 0.05f, 16};
        DevBuf counts;           // uint8 [n_seq][h_top][w_top]
    } fuse;
    int set_keyframe_fusion(const dvo_kf_fusion_config* c);  // (validated by the caller)
    int fuse_keyframes(int frame_set, int kf);
    // Keyframe carry (dvo_batch_set_keyframe_carry): on a promotion k_kf_carry blends the old keyframe's fused depth,
    // warped into the tracked frame, into the tracked set's depth pyramid before k_promote copies it, and the counts follow through a
    // staging plane (k_kf_carry_commit, after k_kf_fuse has cleared).  Needs fusion; off (the default): no launch is added.
    struct KfCarry : KfStage {
        dvo_kf_carry_config cfg = {(int)sizeof(dvo_kf_carry_config), DVO_KF_CARRY_OFF, 0.05f};
        DevBuf staged;           // uint8 [n_seq][h_top][w_top]
    } carry;
    int set_keyframe_carry(const dvo_kf_carry_config* c);    // (validated by the caller)
    bool carry_keyframes(int frame_set, int kf);             // carry prep + carry; true when the commit has to follow the fusion
    void commit_carry();
    KfPrepArgs kf_prep_args(const KfStage& st) const;
    // what KfFuseArgs and KfCarryArgs share: geometry, intrinsics, thresholds, the stage's table and records (max_diff is the stage's own)
    template <class Args> void kf_pixel_args(Args& a, const KfStage& st, float max_diff) const;
    PointsExport points;                                     // dvo_batch_export_points (keyframe tracking)
    PointsExport::Source points_source(int level) const;
};

int select_device(int device);
// true when `p` is page-locked host memory known to HIP (hipHostMalloc / hipHostRegister): only then may an asynchronous copy
// still read the buffer after the call that queued it has returned
bool host_buffer_is_pinned(const void* p);

// Optional roctx ranges (the reference prints a Timer line per Gauss-Newton iteration and mapping stage: tracker.cpp:43,54-61,
// mapper.cpp:18,27,32): with DVO_TRACE=1 in the environment every tracking level and mapping stage of a frame is a named range in a
// `rocprofv3 --marker-trace` timeline.  libroctx64 is loaded lazily with dlopen; without it, or without DVO_TRACE, these are no-ops.
void trace_push(const char* name);
void trace_pop();
struct TraceRange { explicit TraceRange(const char* n) { trace_push(n); } ~TraceRange() { trace_pop(); } };

// n_seq independent MONO sequences on one GPU: System::VisualOdometry::odometrize (system.hpp:44-74) -- track against the newest
// keyframe, then Mapper::estimate (propagate + new keyframe, or stereo update) and regularize -- for every sequence per call, with
// the keyframe decision taken on the device per sequence.  FrameHistory is a ring of the newest R keyframes per sequence
// (their top-level gray + pose; the reference keeps every frame forever, frame.hpp:146-188): with R >= the number of keyframes
// a run creates the results equal the reference's unbounded history, beyond that a dvo_vo handle with history limit R.
struct MonoBatch {
    int n_seq = 0, device = 0, R = 8;
    dvo_config cfg;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Geometry g;              // Frame(gray, K, 3, 2), system.hpp:47
    Tracker trk;
    FrameSet ref, frm;       // newest keyframe of every sequence; the frame being processed
    DevBuf ref_age, frm_age, owner, tmp, ring_gray, hist_xi, ages, meta, init_depth, init_sigma;
    DevBuf xi_world, T_world, is_key;
    DevBuf need_list;        // [0] = number of sequences that create a keyframe on this frame, [4..] their ids (k_mono_decide)
    float* depth_alt = nullptr;  // the second top-level depth buffer of `ref` (k_regularize_redecimate ping-pongs between the two)
    int latest_id = -1;      // Frame::latest_id, frame.cpp:5 (all sequences advance in lockstep); with actions: calls made - 1
                             // (each sequence's own frame id is then MonoSeq::frame_id)
    bool have_init = false;
    // Per-camera batch (dvo_batch_create_mono_cameras): [level][n_seq] Intr (the tracker's table, Tracker::cam_k; its top-level row
    // is the mapping kernels' Intr), then [n_seq] MapK (culled top-level K9 + k_sparse).  Fixed at creation.  Empty: one K.
    DevBuf cam_dev;
    const Intr* cam_top() const { return cam_dev.p ? cam_dev.as<Intr>() + (size_t)g.top() * n_seq : nullptr; }
    const MapK* cam_map() const { return cam_dev.p ? reinterpret_cast<const MapK*>(cam_dev.as<Intr>() + (size_t)g.levels * n_seq) : nullptr; }
    std::vector<float> K_full;   // the creation K at full resolution: [9], or (per camera) [n_seq][9] -- the undistortion's camera
    Undistortion und;            // dvo_batch_set_distortion (before the first frame)
    int set_distortion(const float* D, bool per_sequence);
    Photometry pho;              // dvo_batch_set_photometric (before the first frame)
    int set_photometric(int n_cal, const float* resp, const float* vign, const int* seq_cal);
    PyramidKernel last_build;    // what the last frame build launched (dvo_debug_batch_last_pyramid_kernel)
    // K: [9] for every sequence, or (per_camera) [n][9], one per sequence
    int init(int n, const float* K, int w, int h, int ring, const dvo_config* c, bool per_camera = false);
    ~MonoBatch();
    int set_initial_depth(const float* depth_host, const float* sigma_host);              // one map, broadcast to every sequence
    int set_initial_depth_device(const float* depth_dev, const float* sigma_dev);         // [n_seq][th][tw]
    int odometrize(const FrameInput& in);                                                  // gray [n_seq][h][w] float, or raw u8
    int odometrize_host(const void* frames, FrameInput in);                                // the same from host memory (copy stream, 2 slots)
    HostStage host;          // (one map per frame)
    int top_pixels() const { return g.w[g.top()] * g.h[g.top()]; }
    // profiling of the mapping stages (cfg.profile): hipEvent pairs on `stream` around k_depth_update (+ k_age_table),
    // k_regularize_redecimate and the three k_propagate_* passes of every frame
    struct MapEv { hipEvent_t e[6]; };
    std::vector<MapEv> map_ev;
    size_t map_ev_used = 0;
    double prof_update_ms = 0, prof_regularize_ms = 0, prof_propagate_ms = 0;
    uint64_t prof_frames = 0;
    int collect_map_profile();
    int queue_depth_update(int frame_id, MapEv* pe);   // k_age_table + k_depth_update[_cam] of one frame (pe: profiling events or nullptr)
    // Per-sequence skip / restart (dvo_batch_set_mono_actions).  Allocated on first use; a batch that never sets
    // actions runs the plain path.  k_plan resolves the actions with plan.has_ref = "has a keyframe"; started = has started before (the
    // first start keeps the slot's own initial maps); need_save parks MonoSeq::need of the sequences that do not track.
    SeqPlan plan;
    DevBuf started, need_save;
    const float* start_depth = nullptr;         // start maps of the next call (dvo_batch_set_mono_start_depth_device)
    const float* start_sigma = nullptr;
    bool host_init = false;                     // init_depth holds the host map of set_initial_depth (else, once planned, the default)
    int alloc_plan();
    int set_actions(const uint8_t* actions, bool on_device);
    int set_start_depth(const float* depth_dev, const float* sigma_dev);
    int status_of_last(int* out, bool out_on_device);
    int odometrize_planned(const FrameInput& gin, int call_id);
    int started_of(int seq, bool* out);         // (synchronises) whether sequence `seq` has a keyframe
    PoseGuess guess;                            // dvo_batch_set_pose_guess_mode / dvo_batch_set_pose_guess (world twists)
    int set_guess_mode(int mode);
    TrackQuality quality;                       // dvo_batch_set_track_quality
    PointsExport points;                        // dvo_batch_export_points
    PointsExport::Source points_source(int level) const;
};

void default_initial_depth(int n, uint32_t seed, std::vector<float>& d, std::vector<float>& s);

}  // namespace dvo

// the C handle behind dvo_batch*: a sensor-depth batch (impl) or, when `mono` is set, a mono track + map batch
struct dvo_batch {
    dvo::Batch impl;
    std::unique_ptr<dvo::MonoBatch> mono;
    // what both kinds have, of whichever is live
    int device() const { return mono ? mono->device : impl.device; }
    hipStream_t stream() const { return mono ? mono->stream : impl.stream; }
    int n_seq() const { return mono ? mono->n_seq : impl.n_seq; }
    dvo::Tracker& trk() { return mono ? mono->trk : impl.trk; }
    dvo::PoseGuess& guess() { return mono ? mono->guess : impl.guess; }
    dvo::TrackQuality& quality() { return mono ? mono->quality : impl.quality; }
    dvo::SeqPlan& plan() { return mono ? mono->plan : impl.plan; }
    int pushes() const { return mono ? mono->latest_id + 1 : impl.n_push; }   // pushes / calls that consumed a frame
};
