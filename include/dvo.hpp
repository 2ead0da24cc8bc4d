// dvo.hpp -- header-only C++17 facade over the C ABI of libdvo.so (include/dvo.h).
//
// Mirrors the public surface of the reference's System::VisualOdometry (include/system/system.hpp:12-104):
// the same three entry points (constructor from K, odometrize, odometrizeUsingDepth) plus keyframe / depth-map
// access (include/system/frame.hpp:125-139,146-188).  Images are row-major float buffers instead of cv::Mat1f;
// INTEGRATION.md shows the cv::Mat adaptor a maintainer of the reference would write on top of this.
// Errors surface as dvo::Error (the reference abort()s or throws std::out_of_range).
#pragma once
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "dvo.h"

namespace dvo {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

inline void check(int st)
{
    if (st != DVO_OK) throw Error(st, std::string(dvo_status_string(st)) + ": " + dvo_last_error());
}

using Mat4 = std::array<float, 16>;  // row-major 4x4 pose
using Vec6 = std::array<float, 6>;   // twist (vx, vy, vz, wx, wy, wz), src/math/se3.cpp:74-75
using Mat3 = std::array<float, 9>;   // row-major intrinsics

inline dvo_config default_config()
{
    dvo_config c;
    dvo_config_default(&c);
    return c;
}

struct Keyframe {  // one level of a System::Frame (include/system/frame.hpp:72-144)
    int id = -1, levels = 0, level = 0, width = 0, height = 0;
    Vec6 xi{}, relative_xi{};
    Mat3 K{};
    std::vector<float> gray, depth, sigma, age;  // age only on the top level
};

class VisualOdometry {
public:
    // VisualOdometry(const cv::Mat1f& K), system.hpp:15
    VisualOdometry(const Mat3& K, int width, int height, const dvo_config* cfg = nullptr) : w_(width), h_(height)
    {
        check(dvo_vo_create(K.data(), width, height, cfg, &vo_));
    }
    // VisualOdometry(gray, depth, sigma, K), system.hpp:24-32
    VisualOdometry(const float* gray, const float* depth, const float* sigma, const Mat3& K, int width, int height,
                   const dvo_config* cfg = nullptr)
        : VisualOdometry(K, width, height, cfg)
    {
        check(dvo_vo_init_keyframe(vo_, gray, depth, sigma));
    }
    ~VisualOdometry() { dvo_vo_destroy(vo_); }
    VisualOdometry(const VisualOdometry&) = delete;
    VisualOdometry& operator=(const VisualOdometry&) = delete;

    // replaces the cv::randn initial depth (include/system/frame.hpp:17-21): maps at width/4 x height/4
    void setInitialDepth(const float* depth, const float* sigma) { check(dvo_vo_set_initial_depth(vo_, depth, sigma)); }
    // Loader::getNormalizedUndistortedImages (src/core/loader.cpp:15-42) fused into odometrize / odometrizeRaw: D = (k1, k2, p1, p2, k3)
    // with the creation K, before the first frame (dvo_vo_set_distortion)
    void setDistortion(const std::array<float, 5>& D) { check(dvo_vo_set_distortion(vo_, D.data())); }
    // photometric calibration of every raw mono frame, before the first one: invResponse[256] (nullptr: i / 255), vignette
    // [height][width] (nullptr: 1); both nullptr clears (dvo_vo_set_photometric).  From then on feed raw frames.
    void setPhotometric(const float* invResponse, const float* vignette) { check(dvo_vo_set_photometric(vo_, invResponse, vignette)); }

    // cv::Mat1f odometrize(const cv::Mat1f& gray), system.hpp:44-74: 4x4 world pose exp(m_xi)
    Mat4 odometrize(const float* gray, bool* is_keyframe = nullptr)
    {
        Mat4 T;
        int key = 0;
        check(dvo_vo_odometrize(vo_, gray, T.data(), &key));
        if (is_keyframe) *is_keyframe = key != 0;
        return T;
    }
    // the same from a raw u8 frame (gray / R,G,B / R,G,B,A), converted on the device
    Mat4 odometrizeRaw(const uint8_t* rgb, int channels, bool* is_keyframe = nullptr)
    {
        Mat4 T;
        int key = 0;
        check(dvo_vo_odometrize_raw(vo_, rgb, channels, T.data(), &key));
        if (is_keyframe) *is_keyframe = key != 0;
        return T;
    }
    // cv::Mat1f odometrizeUsingDepth(gray, depth, sigma), system.hpp:77-93: 4x4 relative pose
    Mat4 odometrizeUsingDepth(const float* gray, const float* depth, const float* sigma)
    {
        Mat4 T;
        check(dvo_vo_odometrize_depth(vo_, gray, depth, sigma, T.data()));
        return T;
    }

    // FrameHistory::size / operator[] (frame.hpp:174-176); index 0 = oldest keyframe
    int keyframeCount() const { return dvo_vo_keyframe_count(vo_); }
    Keyframe keyframe(int index, int level = -1) const
    {
        Keyframe k;
        int tw = 0, th = 0;
        check(dvo_vo_keyframe_info(vo_, index, &k.id, &k.levels, &tw, &th, k.xi.data(), k.relative_xi.data()));
        k.level = level < 0 ? k.levels - 1 : level;
        const int shift = k.levels - 1 - k.level;
        k.width = tw >> shift;
        k.height = th >> shift;
        const size_t n = (size_t)k.width * k.height;
        k.gray.resize(n); k.depth.resize(n); k.sigma.resize(n);
        float* age = nullptr;
        if (shift == 0) { k.age.resize(n); age = k.age.data(); }
        check(dvo_vo_keyframe_get(vo_, index, k.level, k.gray.data(), k.depth.data(), k.sigma.data(), age, k.K.data()));
        return k;
    }
    dvo_track_log lastTrackLog() const
    {
        dvo_track_log log;
        check(dvo_vo_last_track_log(vo_, &log));
        return log;
    }
    int width() const { return w_; }
    int height() const { return h_; }
    dvo_vo* handle() { return vo_; }

private:
    dvo_vo* vo_ = nullptr;
    int w_, h_;
};

// n_seq independent sequences on one GPU (frame-to-frame tracking with sensor depth, or keyframe tracking: setKeyframeTracking)
class BatchTracker {
public:
    BatchTracker(int n_seq, const Mat3& K, int width, int height, int levels = 4, int culls = 1, const dvo_config* cfg = nullptr)
        : n_(n_seq), w_(width), h_(height), levels_(levels), culls_(culls)
    {
        check(dvo_batch_create(n_seq, K.data(), width, height, levels, culls, cfg, &b_));
    }
    ~BatchTracker() { dvo_batch_destroy(b_); }
    BatchTracker(const BatchTracker&) = delete;
    BatchTracker& operator=(const BatchTracker&) = delete;
    void pushDevice(const float* gray, const float* depth, const float* sigma) { check(dvo_batch_push_device(b_, gray, depth, sigma)); }
    void pushHost(const float* gray, const float* depth, const float* sigma) { check(dvo_batch_push_host(b_, gray, depth, sigma)); }
    // raw sensor frames as cv::imread delivers them (u8 gray / RGB(A), u16 depth): converted inside the pyramid kernel
    void pushRawDevice(const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale = 0.0f)
    { check(dvo_batch_push_raw_device(b_, rgb, channels, depth16, depth_scale)); }
    void pushRawHost(const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale = 0.0f)
    { check(dvo_batch_push_raw_host(b_, rgb, channels, depth16, depth_scale)); }
    std::vector<Vec6> lastTwists()
    {
        std::vector<Vec6> out(n_);
        check(dvo_batch_last_poses(b_, out[0].data(), nullptr));
        return out;
    }
    std::vector<Mat4> lastPoses()
    {
        std::vector<Mat4> out(n_);
        check(dvo_batch_last_poses(b_, nullptr, out[0].data()));
        return out;
    }
    // per-sequence action of the next push (DVO_SEQ_SKIP / TRACK / RESTART, [n_seq]; nullptr clears), see dvo_batch_set_actions
    void setActions(const uint8_t* actions, bool onDevice = false) { check(dvo_batch_set_actions(b_, actions, onDevice ? 1 : 0)); }
    // per-sequence outcome of the last push (DVO_SEQ_TRACKED / SKIPPED / STARTED / BAD_ACTION)
    std::vector<int> lastStatus()
    {
        std::vector<int> out(n_);
        check(dvo_batch_last_status(b_, out.data()));
        return out;
    }
    void copyStatusDevice(int* statusDev) { check(dvo_batch_copy_status_device(b_, statusDev)); }
    // start pose of the tracking (DVO_GUESS_NONE / GIVEN / CONSTANT_VELOCITY), see dvo_batch_set_pose_guess_mode
    void setPoseGuessMode(int mode) { check(dvo_batch_set_pose_guess_mode(b_, mode)); }
    // relative twists [n_seq][6] of the next push (DVO_GUESS_GIVEN; nullptr clears)
    void setPoseGuess(const float* xi, bool onDevice = false) { check(dvo_batch_set_pose_guess(b_, xi, onDevice ? 1 : 0)); }
    std::vector<std::array<float, 6>> lastStartPoses()
    {
        std::vector<std::array<float, 6>> out(n_);
        check(dvo_batch_last_start_poses(b_, out[0].data()));
        return out;
    }
    // per-sequence tracking quality of the last push (dvo_batch_set_track_quality): records [n_seq], host (synchronises) or device
    void setTrackQuality(bool enable = true) { check(dvo_batch_set_track_quality(b_, enable ? 1 : 0)); }
    std::vector<dvo_track_quality> lastTrackQuality()
    {
        std::vector<dvo_track_quality> out(n_);
        check(dvo_batch_last_track_quality(b_, out.data()));
        return out;
    }
    void copyTrackQualityDevice(dvo_track_quality* dst) { check(dvo_batch_copy_track_quality_device(b_, dst)); }
    // robust residual weights from the next push / call on (dvo_batch_set_robust_weights): kind DVO_ROBUST_NONE turns them off
    void setRobustWeights(int kind, float param = 1.345f, int scale_mode = DVO_ROBUST_SCALE_ADAPTIVE, float scale_floor = 1e-3f)
    {
        dvo_robust_config c{(int)sizeof(dvo_robust_config), kind, scale_mode, param, scale_floor};
        check(dvo_batch_set_robust_weights(b_, &c));
    }
    void setRobustScales(const float* s, bool onDevice = false) { check(dvo_batch_set_robust_scales(b_, s, onDevice ? 1 : 0)); }
    std::vector<float> lastRobustScales()
    {
        std::vector<float> out(n_);
        check(dvo_batch_last_robust_scales(b_, out.data()));
        return out;
    }
    // robust weights with the median (MAD) scale from the next push / call on (dvo_batch_set_robust_median): kind DVO_ROBUST_HUBER or
    // DVO_ROBUST_STUDENT_T; setRobustWeights(DVO_ROBUST_NONE) turns them off
    void setRobustMedian(int kind, float param = 1.345f, float scale_floor = 1e-3f)
    {
        dvo_robust_config c{(int)sizeof(dvo_robust_config), kind, DVO_ROBUST_SCALE_MEDIAN, param, scale_floor};
        check(dvo_batch_set_robust_median(b_, &c));
    }
    dvo_robust_log lastRobustLog(int seq)
    {
        dvo_robust_log lg{};
        lg.struct_size = (int)sizeof(dvo_robust_log);
        check(dvo_batch_last_robust_log(b_, seq, &lg));
        return lg;
    }
    std::vector<uint32_t> lastRobustHistogram(int seq)
    {
        std::vector<uint32_t> out(256);
        check(dvo_batch_last_robust_histogram(b_, seq, out.data()));
        return out;
    }
    // affine brightness compensation from the next push / call on (dvo_batch_set_affine_brightness): mode DVO_AFFINE_OFF turns it off
    void setAffineBrightness(int mode, int min_pixels = 64, float min_contrast = 1e-3f, float gain_min = 0.25f, float gain_max = 4.0f)
    {
        dvo_affine_config c{(int)sizeof(dvo_affine_config), mode, min_pixels, min_contrast, gain_min, gain_max};
        check(dvo_batch_set_affine_brightness(b_, &c));
    }
    void setAffineRows(const float* ab, bool onDevice = false) { check(dvo_batch_set_affine_rows(b_, ab, onDevice ? 1 : 0)); }
    std::vector<float> lastAffine()   // [n_seq][2]
    {
        std::vector<float> out(2 * (size_t)n_);
        check(dvo_batch_last_affine(b_, out.data()));
        return out;
    }
    dvo_affine_log lastAffineLog(int seq)
    {
        dvo_affine_log lg{};
        lg.struct_size = (int)sizeof lg;
        check(dvo_batch_last_affine_log(b_, seq, &lg));
        return lg;
    }
    // the geometric (depth) term from the next push on (dvo_batch_set_geometric): mode DVO_GEOMETRIC_OFF turns it off
    void setGeometric(int mode = DVO_GEOMETRIC_ON, float weight = 10.0f, float max_diff = 0.1f)
    {
        dvo_geometric_config c{(int)sizeof(dvo_geometric_config), mode, weight, max_diff};
        check(dvo_batch_set_geometric(b_, &c));
    }
    // both together from the next push on (dvo_batch_set_geometric_affine); setGeometric(OFF) / setAffineBrightness(OFF) turn either off
    void setGeometricAffine(float weight = 10.0f, float max_diff = 0.1f, int affine_mode = DVO_AFFINE_ESTIMATE, int min_pixels = 64,
                            float min_contrast = 1e-3f, float gain_min = 0.25f, float gain_max = 4.0f)
    {
        dvo_geometric_config g{(int)sizeof(dvo_geometric_config), DVO_GEOMETRIC_ON, weight, max_diff};
        dvo_affine_config a{(int)sizeof(dvo_affine_config), affine_mode, min_pixels, min_contrast, gain_min, gain_max};
        check(dvo_batch_set_geometric_affine(b_, &g, &a));
    }
    std::vector<dvo_geometric_record> lastGeometric()   // [n_seq]
    {
        std::vector<dvo_geometric_record> out(n_);
        check(dvo_batch_last_geometric(b_, out.data()));
        return out;
    }
    dvo_geometric_log lastGeometricLog(int seq)
    {
        dvo_geometric_log lg{};
        lg.struct_size = (int)sizeof lg;
        check(dvo_batch_last_geometric_log(b_, seq, &lg));
        return lg;
    }
    // step control from the next push / call on (dvo_batch_set_step_control): damped Gauss-Newton with step acceptance; DVO_LM_OFF turns it off
    void setStepControl(int mode = DVO_LM_ON, float lambda0 = 1.0f, float lambda_up = 4.0f, float lambda_down = 0.5f, float lambda_floor = 1e-4f,
                        float lambda_max = 1e6f, float min_valid_fraction = 0.5f)
    {
        dvo_lm_config c{(int)sizeof(dvo_lm_config), mode, lambda0, lambda_up, lambda_down, lambda_floor, lambda_max, min_valid_fraction};
        check(dvo_batch_set_step_control(b_, &c));
    }
    std::vector<dvo_lm_record> lastStepControl()   // [n_seq]
    {
        std::vector<dvo_lm_record> out(n_);
        check(dvo_batch_last_step_control(b_, out.data()));
        return out;
    }
    dvo_lm_log lastStepControlLog(int seq)
    {
        dvo_lm_log lg{};
        lg.struct_size = (int)sizeof lg;
        check(dvo_batch_last_step_control_log(b_, seq, &lg));
        return lg;
    }
    // per-sequence camera intrinsics from the next push on ([n_seq]; nullptr: the creation K for every sequence), see dvo_batch_set_intrinsics
    void setIntrinsics(const Mat3* K) { check(dvo_batch_set_intrinsics(b_, K ? K[0].data() : nullptr)); }
    std::vector<Mat3> intrinsics()
    {
        std::vector<Mat3> out(n_);
        check(dvo_batch_get_intrinsics(b_, out[0].data()));
        return out;
    }
    // lens undistortion of every frame from the next push on: D[5] for every sequence, or (perSequence) D[n_seq][5]; nullptr clears
    // (dvo_batch_set_sensor_distortion).  distortion(): the [n_seq][5] coefficients the next push uses (empty when none).
    void setDistortion(const float* D, bool perSequence = false) { check(dvo_batch_set_sensor_distortion(b_, D, perSequence ? 1 : 0)); }
    // the gray pyramid of every frame low-pass filtered before each halving (DVO_PYRAMID_FILTER_BINOMIAL3) or decimated (_NONE, the
    // default); before the first push or prefetch, not together with setDistortion (dvo_batch_set_pyramid_filter)
    void setPyramidFilter(int filter = DVO_PYRAMID_FILTER_BINOMIAL3) { check(dvo_batch_set_pyramid_filter(b_, filter)); }
    int pyramidFilter()
    {
        int f = DVO_PYRAMID_FILTER_NONE;
        check(dvo_batch_pyramid_filter(b_, &f));
        return f;
    }
    std::vector<std::array<float, 5>> distortion()
    {
        std::vector<std::array<float, 5>> D(n_);
        int enabled = 0;
        check(dvo_batch_get_sensor_distortion(b_, D[0].data(), &enabled));
        if (!enabled) D.clear();
        return D;
    }
    // track each frame against its sequence's keyframe instead of the previous frame, before the first push (dvo_batch_set_keyframe_tracking)
    void setKeyframeTracking(bool enable = true) { check(dvo_batch_set_keyframe_tracking(b_, enable ? 1 : 0)); }
    // with keyframe tracking: fold every tracked frame's depth into its keyframe's map from the next push on (dvo_batch_set_keyframe_fusion);
    // mode DVO_KF_FUSION_OFF stops and leaves the maps as they are
    void setKeyframeFusion(int mode = DVO_KF_FUSION_ON, float max_diff = 0.05f, int max_count = 16)
    {
        dvo_kf_fusion_config c{mode, max_diff, max_count};
        check(dvo_batch_set_keyframe_fusion(b_, &c));
    }
    std::vector<dvo_kf_fusion_record> lastKeyframeFusion()   // [n_seq]
    {
        std::vector<dvo_kf_fusion_record> out(n_);
        check(dvo_batch_last_keyframe_fusion(b_, out.data()));
        return out;
    }
    std::vector<uint8_t> keyframeFusionCounts(int seq)   // [h_top][w_top]
    {
        std::vector<uint8_t> out((size_t)(w_ >> culls_) * (size_t)(h_ >> culls_));
        check(dvo_batch_keyframe_fusion_counts(b_, seq, out.data()));
        return out;
    }
    // with keyframe fusion: carry the fused depth and the counts into the next keyframe at every promotion from the next push on
    // (dvo_batch_set_keyframe_carry); mode DVO_KF_CARRY_OFF stops and leaves maps and counts as they are
    void setKeyframeCarry(int mode = DVO_KF_CARRY_ON, float max_diff = 0.05f)
    {
        dvo_kf_carry_config c{(int)sizeof(dvo_kf_carry_config), mode, max_diff};
        check(dvo_batch_set_keyframe_carry(b_, &c));
    }
    std::vector<dvo_kf_carry_record> lastKeyframeCarry()   // [n_seq]
    {
        std::vector<dvo_kf_carry_record> out(n_);
        check(dvo_batch_last_keyframe_carry(b_, out.data()));
        return out;
    }
    // with keyframe tracking: the keyframe maps as compacted world-frame points in the caller's DEVICE buffers (dvo_batch_export_points:
    // asynchronous on the handle's stream; cfg from dvo_points_config_default); lastPoints: the offsets of that export (synchronises)
    void exportPoints(const dvo_points_config& cfg, uint32_t capacity, float* xyzg_dev, uint32_t* src_dev, uint32_t* offsets_dev)
    {
        check(dvo_batch_export_points(b_, &cfg, capacity, xyzg_dev, src_dev, nullptr, offsets_dev));
    }
    std::vector<uint32_t> lastPoints()   // [n_seq + 1]
    {
        std::vector<uint32_t> out((size_t)n_ + 1);
        check(dvo_batch_last_points(b_, out.data()));
        return out;
    }
    // with keyframe tracking: world poses of the last push (and its keyframe flags), as BatchMono::worldPoses
    std::vector<Mat4> worldPoses(std::vector<int>* is_keyframe = nullptr)
    {
        std::vector<Mat4> out(n_);
        if (is_keyframe) is_keyframe->resize(n_);
        check(dvo_batch_world_poses(b_, nullptr, out[0].data(), is_keyframe ? is_keyframe->data() : nullptr));
        return out;
    }
    // asynchronous device-to-device copies on the handle's stream: [n_seq][6], [n_seq][16], [n_seq]; any may be nullptr
    void copyWorldPosesDevice(float* xiDev, float* TDev = nullptr, int* keyDev = nullptr) { check(dvo_batch_copy_world_poses_device(b_, xiDev, TDev, keyDev)); }
    // the keyframe of sequence `seq`: gray and depth of one level (default: the finest), its world twist and id (no sigma or age)
    Keyframe keyframe(int seq, int level = -1)
    {
        Keyframe k;
        k.levels = levels_;
        k.level = level < 0 ? levels_ - 1 : level;
        if (k.level >= levels_) throw Error(DVO_ERR_BAD_ARGUMENT, "BatchTracker::keyframe: level " + std::to_string(level) + " is outside [0, levels)");
        const int shift = culls_ + (levels_ - 1 - k.level);
        k.width = w_ >> shift;
        k.height = h_ >> shift;
        const size_t n = (size_t)k.width * k.height;
        k.gray.resize(n); k.depth.resize(n);
        int n_keyframes = 0, valid = 0;
        check(dvo_batch_keyframe_get(b_, seq, k.level, k.gray.data(), k.depth.data(), nullptr, nullptr, k.xi.data(), &k.id, &n_keyframes, &valid));
        return k;
    }
    dvo_batch* handle() { return b_; }

private:
    dvo_batch* b_ = nullptr;
    int n_, w_, h_, levels_, culls_;
};

// n_seq independent MONO sequences on one GPU: System::VisualOdometry::odometrize (system.hpp:44-74: track + Mapper::estimate +
// regularize) for every sequence per call; Mapper::needNewFrame (src/map/mapper.cpp:45-60) is decided per sequence on the device
class BatchMono {
public:
    BatchMono(int n_seq, const Mat3& K, int width, int height, int ring_keyframes = 8, const dvo_config* cfg = nullptr) : n_(n_seq)
    {
        check(dvo_batch_create_mono(n_seq, K.data(), width, height, ring_keyframes, cfg, &b_));
    }
    // one K per sequence (K[n_seq], fixed at creation), see dvo_batch_create_mono_cameras
    BatchMono(int n_seq, const Mat3* K, int width, int height, int ring_keyframes = 8, const dvo_config* cfg = nullptr) : n_(n_seq)
    {
        check(dvo_batch_create_mono_cameras(n_seq, K ? K[0].data() : nullptr, width, height, ring_keyframes, cfg, &b_));
    }
    ~BatchMono() { dvo_batch_destroy(b_); }
    BatchMono(const BatchMono&) = delete;
    BatchMono& operator=(const BatchMono&) = delete;
    void setInitialDepth(const float* depth, const float* sigma) { check(dvo_batch_set_initial_depth(b_, depth, sigma)); }
    // lens undistortion of every frame, before the first one: D[5] for every sequence, or (perSequence) D[n_seq][5]; nullptr clears
    // (dvo_batch_set_distortion).  distortion(): the [n_seq][5] coefficients in use (empty when none).
    void setDistortion(const float* D, bool perSequence = false) { check(dvo_batch_set_distortion(b_, D, perSequence ? 1 : 0)); }
    std::vector<std::array<float, 5>> distortion()
    {
        std::vector<std::array<float, 5>> D(n_);
        int enabled = 0;
        check(dvo_batch_get_distortion(b_, D[0].data(), &enabled));
        if (!enabled) D.clear();
        return D;
    }
    // photometric calibration of every raw frame, before the first one: nCal inverse-response tables [nCal][256] (nullptr: i / 255)
    // and vignettes [nCal][height][width] (nullptr: 1), seqCal[n_seq] picks each sequence's (nullptr: 0); nCal = 0 clears
    // (dvo_batch_set_photometric).  From then on only raw frames are accepted.
    void setPhotometric(int nCal, const float* invResponse, const float* vignette, const int* seqCal = nullptr)
    {
        check(dvo_batch_set_photometric(b_, nCal, invResponse, vignette, seqCal));
    }
    void odometrizeDevice(const float* gray) { check(dvo_batch_odometrize_device(b_, gray)); }
    void odometrizeRawDevice(const uint8_t* rgb, int channels) { check(dvo_batch_odometrize_raw_device(b_, rgb, channels)); }
    // per-sequence action of the next call (DVO_SEQ_SKIP / TRACK / RESTART; nullptr clears), see dvo_batch_set_mono_actions
    void setActions(const uint8_t* actions, bool onDevice = false) { check(dvo_batch_set_mono_actions(b_, actions, onDevice ? 1 : 0)); }
    // per-sequence outcome of the last call (DVO_SEQ_TRACKED / SKIPPED / STARTED / BAD_ACTION)
    std::vector<int> lastStatus()
    {
        std::vector<int> out(n_);
        check(dvo_batch_mono_last_status(b_, out.data()));
        return out;
    }
    void copyStatusDevice(int* statusDev) { check(dvo_batch_copy_mono_status_device(b_, statusDev)); }
    // start maps [n_seq][height/4][width/4] (device) of the sequences that start in the next call; nullptr, nullptr clears
    void setStartDepthDevice(const float* depthDev, const float* sigmaDev) { check(dvo_batch_set_mono_start_depth_device(b_, depthDev, sigmaDev)); }
    // start pose of the tracking (DVO_GUESS_NONE / GIVEN / CONSTANT_VELOCITY), see dvo_batch_set_pose_guess_mode
    void setPoseGuessMode(int mode) { check(dvo_batch_set_pose_guess_mode(b_, mode)); }
    // world twists [n_seq][6] of the next call (DVO_GUESS_GIVEN; nullptr clears)
    void setPoseGuess(const float* xi, bool onDevice = false) { check(dvo_batch_set_pose_guess(b_, xi, onDevice ? 1 : 0)); }
    std::vector<std::array<float, 6>> lastStartPoses()
    {
        std::vector<std::array<float, 6>> out(n_);
        check(dvo_batch_last_start_poses(b_, out[0].data()));
        return out;
    }
    // per-sequence tracking quality of the last call (dvo_batch_set_track_quality): records [n_seq], host (synchronises) or device
    void setTrackQuality(bool enable = true) { check(dvo_batch_set_track_quality(b_, enable ? 1 : 0)); }
    std::vector<dvo_track_quality> lastTrackQuality()
    {
        std::vector<dvo_track_quality> out(n_);
        check(dvo_batch_last_track_quality(b_, out.data()));
        return out;
    }
    void copyTrackQualityDevice(dvo_track_quality* dst) { check(dvo_batch_copy_track_quality_device(b_, dst)); }
    // robust residual weights from the next push / call on (dvo_batch_set_robust_weights): kind DVO_ROBUST_NONE turns them off
    void setRobustWeights(int kind, float param = 1.345f, int scale_mode = DVO_ROBUST_SCALE_ADAPTIVE, float scale_floor = 1e-3f)
    {
        dvo_robust_config c{(int)sizeof(dvo_robust_config), kind, scale_mode, param, scale_floor};
        check(dvo_batch_set_robust_weights(b_, &c));
    }
    void setRobustScales(const float* s, bool onDevice = false) { check(dvo_batch_set_robust_scales(b_, s, onDevice ? 1 : 0)); }
    std::vector<float> lastRobustScales()
    {
        std::vector<float> out(n_);
        check(dvo_batch_last_robust_scales(b_, out.data()));
        return out;
    }
    // robust weights with the median (MAD) scale from the next push / call on (dvo_batch_set_robust_median): kind DVO_ROBUST_HUBER or
    // DVO_ROBUST_STUDENT_T; setRobustWeights(DVO_ROBUST_NONE) turns them off
    void setRobustMedian(int kind, float param = 1.345f, float scale_floor = 1e-3f)
    {
        dvo_robust_config c{(int)sizeof(dvo_robust_config), kind, DVO_ROBUST_SCALE_MEDIAN, param, scale_floor};
        check(dvo_batch_set_robust_median(b_, &c));
    }
    dvo_robust_log lastRobustLog(int seq)
    {
        dvo_robust_log lg{};
        lg.struct_size = (int)sizeof(dvo_robust_log);
        check(dvo_batch_last_robust_log(b_, seq, &lg));
        return lg;
    }
    std::vector<uint32_t> lastRobustHistogram(int seq)
    {
        std::vector<uint32_t> out(256);
        check(dvo_batch_last_robust_histogram(b_, seq, out.data()));
        return out;
    }
    // affine brightness compensation from the next push / call on (dvo_batch_set_affine_brightness): mode DVO_AFFINE_OFF turns it off
    void setAffineBrightness(int mode, int min_pixels = 64, float min_contrast = 1e-3f, float gain_min = 0.25f, float gain_max = 4.0f)
    {
        dvo_affine_config c{(int)sizeof(dvo_affine_config), mode, min_pixels, min_contrast, gain_min, gain_max};
        check(dvo_batch_set_affine_brightness(b_, &c));
    }
    void setAffineRows(const float* ab, bool onDevice = false) { check(dvo_batch_set_affine_rows(b_, ab, onDevice ? 1 : 0)); }
    std::vector<float> lastAffine()   // [n_seq][2]
    {
        std::vector<float> out(2 * (size_t)n_);
        check(dvo_batch_last_affine(b_, out.data()));
        return out;
    }
    dvo_affine_log lastAffineLog(int seq)
    {
        dvo_affine_log lg{};
        lg.struct_size = (int)sizeof lg;
        check(dvo_batch_last_affine_log(b_, seq, &lg));
        return lg;
    }
    // step control from the next push / call on (dvo_batch_set_step_control): damped Gauss-Newton with step acceptance; DVO_LM_OFF turns it off
    void setStepControl(int mode = DVO_LM_ON, float lambda0 = 1.0f, float lambda_up = 4.0f, float lambda_down = 0.5f, float lambda_floor = 1e-4f,
                        float lambda_max = 1e6f, float min_valid_fraction = 0.5f)
    {
        dvo_lm_config c{(int)sizeof(dvo_lm_config), mode, lambda0, lambda_up, lambda_down, lambda_floor, lambda_max, min_valid_fraction};
        check(dvo_batch_set_step_control(b_, &c));
    }
    std::vector<dvo_lm_record> lastStepControl()   // [n_seq]
    {
        std::vector<dvo_lm_record> out(n_);
        check(dvo_batch_last_step_control(b_, out.data()));
        return out;
    }
    dvo_lm_log lastStepControlLog(int seq)
    {
        dvo_lm_log lg{};
        lg.struct_size = (int)sizeof lg;
        check(dvo_batch_last_step_control_log(b_, seq, &lg));
        return lg;
    }
    std::vector<Mat4> worldPoses(std::vector<int>* is_keyframe = nullptr)
    {
        std::vector<Mat4> out(n_);
        if (is_keyframe) is_keyframe->resize(n_);
        check(dvo_batch_world_poses(b_, nullptr, out[0].data(), is_keyframe ? is_keyframe->data() : nullptr));
        return out;
    }
    // the keyframe maps as compacted world-frame points, as BatchTracker::exportPoints (sigma_dev may be set here)
    void exportPoints(const dvo_points_config& cfg, uint32_t capacity, float* xyzg_dev, uint32_t* src_dev, float* sigma_dev, uint32_t* offsets_dev)
    {
        check(dvo_batch_export_points(b_, &cfg, capacity, xyzg_dev, src_dev, sigma_dev, offsets_dev));
    }
    std::vector<uint32_t> lastPoints()   // [n_seq + 1]
    {
        std::vector<uint32_t> out((size_t)n_ + 1);
        check(dvo_batch_last_points(b_, out.data()));
        return out;
    }
    dvo_batch* handle() { return b_; }

private:
    dvo_batch* b_ = nullptr;
    int n_;
};

}  // namespace dvo
