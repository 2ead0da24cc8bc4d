// dvo_mono.cpp -- the batched MONO pipeline (BASELINE config "tracking + inverse-depth filter"): System::VisualOdometry::odometrize
// (include/system/system.hpp:44-74) and Map::Mapper (src/map/mapper.cpp:16-144) for n_seq sequences per call.  One fixed launch
// sequence per frame, no host round trip: every sequence's keyframe decision (Mapper::needNewFrame) is a flag in device memory that
// the mapping kernels test per sequence.  Reference citations: file:line under the reference tree.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <new>
#include <utility>

#include "dvo_engine.h"

namespace dvo {

MonoBatch::~MonoBatch()
{
    host.release();
    for (auto& m : map_ev)
        for (hipEvent_t e : m.e) (void)hipEventDestroy(e);
    plan.release(stream);   // (host staging goes before the stream does: PinnedPair)
    guess.release(stream);
    trk.rob.release(stream);
    trk.aff.release(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

int MonoBatch::collect_map_profile()
{
    DVO_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < map_ev_used; i++) {
        float p = 0, u = 0, r = 0;
        DVO_HIP(hipEventElapsedTime(&p, map_ev[i].e[0], map_ev[i].e[1]));
        DVO_HIP(hipEventElapsedTime(&u, map_ev[i].e[2], map_ev[i].e[3]));
        DVO_HIP(hipEventElapsedTime(&r, map_ev[i].e[4], map_ev[i].e[5]));
        prof_propagate_ms += p; prof_update_ms += u; prof_regularize_ms += r;
        prof_frames++;
    }
    map_ev_used = 0;
    return DVO_OK;
}

int MonoBatch::init(int n, const float* K, int w, int h, int ring, const dvo_config* c, bool per_camera)
{
    const char* who = per_camera ? "dvo_batch_create_mono_cameras" : "dvo_batch_create_mono";
    if (n < 1 || (!K && !per_camera) || w < 64 || h < 64 || ring < 1 || ring > 64) { set_error(std::string(who) + ": bad arguments"); return DVO_ERR_BAD_ARGUMENT; }
    if (per_camera) DVO_TRY(check_intrinsics(who, K, (size_t)n));
    if (c) cfg = *c; else dvo_config_default(&cfg);
    n_seq = n; R = ring; device = cfg.device;
    K_full.assign(K, K + (per_camera ? (size_t)n * 9 : 9));
    DVO_TRY(select_device(device));
    if (cfg.stream) stream = (hipStream_t)cfg.stream;
    else { DVO_HIP(hipStreamCreate(&stream)); own_stream = true; }
    // (per camera: the frame and pyramid shape do not depend on K; the tracker and mapping kernels read the per-sequence tables)
    DVO_TRY(make_geometry(K, w, h, 3, 2, g));  // Frame(gray, K, 3, 2), system.hpp:47
    DVO_TRY(ref.alloc(g, n, cfg));
    DVO_TRY(frm.alloc(g, n, cfg));
    DVO_TRY(trk.init(g, n, cfg));
    if (per_camera) {   // the tables, once: each sequence's K through the steps make_geometry applies to one K (the same bits)
        const size_t ns = (size_t)n, tab = sizeof(Intr) * (size_t)g.levels * ns;
        std::vector<uint8_t> h_cam(tab + sizeof(MapK) * ns);
        Intr* lv_tab = reinterpret_cast<Intr*>(h_cam.data());
        MapK* map_tab = reinterpret_cast<MapK*>(h_cam.data() + tab);
        for (size_t q = 0; q < ns; q++) {
            Intr lv[DVO_MAX_LEVELS];
            float K9[DVO_MAX_LEVELS][9];
            level_intrinsics(K + q * 9, g, lv, K9);
            for (int l = 0; l < g.levels; l++) lv_tab[(size_t)l * ns + q] = lv[l];
            memcpy(map_tab[q].K9, K9[g.top()], sizeof map_tab[q].K9);
            map_tab[q].k_sparse = k9_sparse(map_tab[q].K9);   // (launch_depth_update's test)
        }
        DVO_TRY(cam_dev.alloc(h_cam.size()));
        DVO_HIP(hipMemcpy(cam_dev.p, h_cam.data(), h_cam.size(), hipMemcpyHostToDevice));
        trk.cam_k = cam_dev.as<Intr>();
    }
    const size_t np = (size_t)top_pixels(), all = np * (size_t)n * sizeof(float);
    DVO_TRY(ref_age.alloc(all)); DVO_TRY(frm_age.alloc(all)); DVO_TRY(owner.alloc(all)); DVO_TRY(tmp.alloc(all));
    DVO_TRY(ring_gray.alloc(all * (size_t)R));
    DVO_TRY(hist_xi.alloc(sizeof(float) * 6 * (size_t)R * n));
    DVO_TRY(ages.alloc(sizeof(AgeEntry) * (size_t)R * n));
    DVO_TRY(meta.alloc(sizeof(MonoSeq) * (size_t)n));
    DVO_TRY(init_depth.alloc(np * sizeof(float))); DVO_TRY(init_sigma.alloc(np * sizeof(float)));
    DVO_TRY(xi_world.alloc(sizeof(float) * 6 * (size_t)n));
    DVO_TRY(T_world.alloc(sizeof(float) * 16 * (size_t)n));
    DVO_TRY(is_key.alloc(sizeof(int) * (size_t)n));
    DVO_TRY(need_list.alloc(sizeof(int) * ((size_t)n + 4)));
    DVO_HIP(hipMemset(meta.p, 0, meta.bytes));
    DVO_HIP(hipMemset(hist_xi.p, 0, hist_xi.bytes));
    return DVO_OK;
}

int Undistortion::set(const char* who, const float* Dh, bool per_sequence, int n_seq, const float* K_full, bool per_camera, const Geometry& g,
                      hipStream_t s)
{
    if (!Dh) { D.clear(); dev.release(); n_cam = 0; this->cam_of.clear(); return DVO_OK; }
    const int nd = per_sequence ? n_seq : 1;
    for (int q = 0; q < nd; q++)
        for (int j = 0; j < 5; j++)
            if (!std::isfinite(Dh[(size_t)q * 5 + j])) {
                set_error(std::string(who) + ": distortion coefficient " + std::to_string(j) + " of sequence " + std::to_string(q) + " is not finite");
                return DVO_ERR_BAD_ARGUMENT;
            }
    // one table per distinct (fx, fy, cx, cy, D): the bits of the camera the table is computed from
    std::map<std::array<uint32_t, 9>, int> ids;
    std::vector<UndistortCam> cams;
    std::vector<int> cam_of((size_t)n_seq);
    for (int q = 0; q < n_seq; q++) {
        UndistortCam c;
        c.k = make_intr(K_full + (per_camera ? (size_t)q * 9 : 0));
        memcpy(c.D, Dh + (per_sequence ? (size_t)q * 5 : 0), sizeof c.D);
        std::array<uint32_t, 9> key;
        const float f[9] = {c.k.fx, c.k.fy, c.k.cx, c.k.cy, c.D[0], c.D[1], c.D[2], c.D[3], c.D[4]};
        memcpy(key.data(), f, sizeof f);
        auto it = ids.emplace(key, (int)cams.size());
        if (it.second) cams.push_back(c);
        cam_of[(size_t)q] = it.first->second;
    }
    const int T = g.top(), tw = g.w[T], th = g.h[T];
    const size_t head = ((size_t)n_seq + 3) & ~(size_t)3, tab = (size_t)tw * th * cams.size();
    DevBuf cams_dev;
    DVO_TRY(cams_dev.alloc(sizeof(UndistortCam) * cams.size()));
    DVO_HIP(hipStreamSynchronize(s));   // (the previous tables may still be read by queued work: none before the first frame)
    D.clear(); n_cam = 0;               // (a failure from here on leaves no undistortion rather than a half-built one)
    DVO_TRY(dev.alloc(sizeof(int) * (head + tab)));
    DVO_HIP(hipMemcpyAsync(cams_dev.p, cams.data(), cams_dev.bytes, hipMemcpyHostToDevice, s));
    DVO_HIP(hipMemcpyAsync(dev.p, cam_of.data(), sizeof(int) * (size_t)n_seq, hipMemcpyHostToDevice, s));
    n_cam = (int)cams.size();
    launch_undistort_map(cams_dev.as<UndistortCam>(), n_cam, g.src_w, g.src_h, g.culls, tw, th, dev.as<int>() + head, s);
    DVO_HIP(hipGetLastError());
    DVO_HIP(hipStreamSynchronize(s));   // (cams_dev and cam_of go out of scope)
    D.resize((size_t)n_seq * 5);
    for (int q = 0; q < n_seq; q++) memcpy(&D[(size_t)q * 5], Dh + (per_sequence ? (size_t)q * 5 : 0), 5 * sizeof(float));
    this->cam_of = cam_of;
    return DVO_OK;
}

int MonoBatch::set_distortion(const float* D, bool per_sequence)
{
    if (latest_id >= 0) { set_error("dvo_batch_set_distortion: the batch has consumed a frame (D is fixed from the first frame on)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    DVO_TRY(und.set("dvo_batch_set_distortion", D, per_sequence, n_seq, K_full.data(), K_full.size() > 9, g, stream));
    return pho.rebuild(n_seq, g, und, stream);   // (a calibration set before D: its gains move to the remap's source pixels)
}

int MonoBatch::set_photometric(int n_cal, const float* resp, const float* vign, const int* seq_cal)
{
    if (latest_id >= 0) { set_error("dvo_batch_set_photometric: the batch has consumed a frame (the calibration is fixed from the first frame on)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    return pho.set("dvo_batch_set_photometric", n_cal, resp, vign, seq_cal, n_seq, g, und, stream);
}

int MonoBatch::set_initial_depth(const float* depth_host, const float* sigma_host)
{  // replaces cv::randn(depth, 1.5, 0.5), max(depth, 0.5), sigma = 0.5 of the first mono keyframe (frame.hpp:17-21, D6)
    if (!depth_host || !sigma_host) { set_error("null map"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(device));
    const size_t np = (size_t)top_pixels();
    DVO_HIP(hipMemcpy(init_depth.p, depth_host, np * sizeof(float), hipMemcpyHostToDevice));
    DVO_HIP(hipMemcpy(init_sigma.p, sigma_host, np * sizeof(float), hipMemcpyHostToDevice));
    const int T = g.top();
    launch_broadcast(init_depth.as<float>(), ref.depth[T], (int)np, n_seq, stream);
    launch_broadcast(init_sigma.as<float>(), ref.sigma[T], (int)np, n_seq, stream);
    have_init = true;
    host_init = true;
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int MonoBatch::set_initial_depth_device(const float* depth_dev, const float* sigma_dev)
{
    if (!depth_dev || !sigma_dev) { set_error("null map"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(device));
    const size_t all = (size_t)top_pixels() * n_seq * sizeof(float);
    const int T = g.top();
    DVO_HIP(hipMemcpyAsync(ref.depth[T], depth_dev, all, hipMemcpyDeviceToDevice, stream));
    DVO_HIP(hipMemcpyAsync(ref.sigma[T], sigma_dev, all, hipMemcpyDeviceToDevice, stream));
    have_init = true;
    return DVO_OK;
}

int MonoBatch::odometrize_host(const void* frames, FrameInput in)
{  // frames of every sequence from host memory: H2D on a copy stream into one of two staging slots (HostStage)
    if (!frames) { set_error("null host pointer"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(device));
    trk.adaptive = false;   // (the host must not be held inside track(): the next frame's transfer is queued meanwhile)
    DVO_TRY(host.begin());
    in.rows_decimated = host.decimate(g, und);
    DVO_TRY(host.upload(0, frames, (size_t)g.src_w * (in.raw() ? (size_t)in.channels : sizeof(float)), g, n_seq, in.rows_decimated));
    DVO_TRY(host.end_copy(stream, host_buffer_is_pinned(frames)));
    const DevBuf& buf = host.cur().buf[0];
    if (in.raw()) in.rgb = buf.as<uint8_t>(); else in.gray = buf.as<float>();
    const int rc = odometrize(in);
    // Known difference from Batch::push_host_frame, kept: a refused frame was not consumed, so it is neither counted nor recorded as
    // this slot's last user -- the same staging slot next time, once whatever was queued has drained.
    if (rc != DVO_OK) {
        (void)hipStreamSynchronize(stream);
        return rc;
    }
    DVO_TRY(host.consumed(stream));
    host.advance();
    return DVO_OK;
}

// The !need branch of Mapper::estimate for every sequence: the stereo update of the reference maps against the keyframe each pixel was
// born in (mapper.cpp:76-137) -- k_age_table over the ring, then k_depth_update (k_depth_update_cam in a per-camera batch).  Its own
// function so that dvo_op_depth_update_batch queues exactly what odometrize() queues.
int MonoBatch::queue_depth_update(int frame_id, MapEv* pe)
{
    const int T = g.top(), tw = g.w[T], th = g.h[T];
    MonoSeq* m = meta.as<MonoSeq>();
    AgeTableArgs ta{};
    ta.meta = m; ta.hist_xi = hist_xi.as<float>(); ta.ages = ages.as<AgeEntry>(); ta.n_seq = n_seq; ta.R = R; ta.n_hist = -1;
    if (pe) DVO_HIP(hipEventRecord(pe->e[2], stream));
    launch_age_table(ta, stream);
    UpdateArgs a{};
    a.ref_depth = ref.depth[T]; a.ref_sigma = ref.sigma[T]; a.ref_age = ref_age.as<float>();
    a.obj_gray = frm.gray[T];
    a.ages = ages.as<AgeEntry>();
    a.ring_gray = ring_gray.as<float>(); a.meta = m;
    a.n_seq = n_seq; a.R = R; a.w = tw; a.h = th; a.crop = cfg.crop_enable; a.obj_id = frame_id;
    a.clamp_age = 1;
    a.seed = cfg.rng_seed;
    a.k = g.k[T];
    memcpy(a.K9, g.K9[T], sizeof a.K9);
    a.seq_k = cam_top(); a.seq_K9 = cam_map();   // (per-camera batch: k_depth_update_cam)
    launch_depth_update(a, stream);
    if (pe) DVO_HIP(hipEventRecord(pe->e[3], stream));
    return DVO_OK;
}

int MonoBatch::odometrize(const FrameInput& in)
{  // system.hpp:44-74 for every sequence
    if (!in.key0() || (in.raw() && in.channels != 1 && in.channels != 3 && in.channels != 4)) { set_error("null device pointer / bad channel count"); return DVO_ERR_BAD_ARGUMENT; }
    if (pho.enabled() && !in.raw()) {
        set_error("the batch has a photometric calibration (dvo_batch_set_photometric), which needs the byte: feed raw frames (dvo_batch_odometrize_raw_device / _raw_host)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    FrameInput gin = in;          // mono: gray only
    gin.depth = nullptr; gin.sigma = nullptr; gin.depth16 = nullptr;
    if (und.enabled() && gin.rows_decimated) { set_error("internal: an undistorted frame needs whole frames"); return DVO_ERR_BAD_ARGUMENT; }
    und.apply(gin, n_seq);        // dvo_batch_set_distortion: k_pyramid_remap
    pho.apply(gin, n_seq);        // dvo_batch_set_photometric: k_pyramid_raw4_photo / k_pyramid_photo
    DVO_TRY(select_device(device));
    const int T = g.top(), tw = g.w[T], th = g.h[T], np = tw * th;
    // Frame::latest_id (frame.cpp:5) advances only once the frame's launches were queued: a call that fails leaves the batch where it
    // was (a failed first frame leaves it not started), so frame ids -- and with them keyframe_max_frames -- never shift
    const int frame_id = latest_id + 1;
    MonoSeq* m = meta.as<MonoSeq>();
    // per-sequence path: actions or start maps pending, or actions used by an earlier call (then every call is an
    // all-TRACK plan).  frame_id is then the number of the call; each sequence counts its own frames in MonoSeq::frame_id.
    const bool planned = plan.act_pending || plan.act_used || start_depth != nullptr;
    if (planned) {
        if (frame_id == 0 && !have_init) {   // the slots' maps of a first start, as the plain first frame sets them
            std::vector<float> d, s;
            default_initial_depth(np, cfg.rng_seed, d, s);
            DVO_TRY(set_initial_depth(d.data(), s.data()));
        }
        DVO_TRY(alloc_plan());
        launch_plan(plan.plan_args(trk, frame_id > 0), stream);   // (no cam_changed: K and D are fixed for the life of the handle)
        if (frame_id == 0 && guess.on()) {   // nothing tracks: the seed only folds the previous call into the history
            const PoseSeedArgs sa = guess.args(trk.state.as<SeqState>(), plan.eff.as<uint8_t>(), 0, xi_world.as<float>(), m);
            launch_mono_seed(sa, stream);
        }
    }
    if (frame_id == 0 && !planned) {  // system.hpp:49-54: the first frame is the first keyframe of every sequence
        if (!have_init) {
            std::vector<float> d, s;
            default_initial_depth(np, cfg.rng_seed, d, s);
            DVO_TRY(set_initial_depth(d.data(), s.data()));
        }
        if (guess.on()) {   // every sequence starts (the seed folds that into the history)
            const PoseSeedArgs sa = guess.args(trk.state.as<SeqState>(), nullptr, DVO_SEQ_RESTART, xi_world.as<float>(), m);
            launch_mono_seed(sa, stream);
        }
        build_pyramid(ref, gin, stream, true, nullptr, nullptr, nullptr, &last_build);
        DVO_HIP(hipMemsetAsync(ref_age.p, 0, ref_age.bytes, stream));
        redecimate(ref, ref.depth[T], ref.sigma[T], stream);
        PromoteArgs pa{};
        pa.n_seq = n_seq; pa.gray_top = ref.gray[T]; pa.ring_gray = ring_gray.as<float>(); pa.npix = np; pa.R = R;
        pa.meta = m; pa.all = 1;
        launch_promote(pa, stream);
        launch_mono_commit(m, hist_xi.as<float>(), n_seq, R, 1, frame_id, xi_world.as<float>(), T_world.as<float>(), is_key.as<int>(), stream);
        DVO_HIP(hipGetLastError());
        guess.given.clear();
        quality.ready = quality.on;
        trk.end_terms(stream);
        latest_id = frame_id;
        return DVO_OK;
    }
    MapEv* pe = nullptr;
    if (cfg.profile) {
        if (map_ev_used == map_ev.size()) {
            MapEv m6;
            for (hipEvent_t& e : m6.e) DVO_HIP(hipEventCreate(&e));
            map_ev.push_back(m6);
        }
        pe = &map_ev[map_ev_used];
    }
    {   // Frame(gray, K, 3, 2); a plan: the SKIP sequences read no input (k_pyramid<true> / k_pyramid_raw4<, true> copy their keyframe's
        // gray forward, k_pyramid_remap_plan writes nothing)
        TraceRange tr("mono pyramid");
        if (planned) build_pyramid(frm, gin, stream, true, plan.eff.as<uint8_t>(), &ref, nullptr, &last_build);
        else build_pyramid(frm, gin, stream, true, nullptr, nullptr, nullptr, &last_build);
    }
    {   // system.hpp:57 (a plan: the TRACK sequences only; before the first call no sequence has a keyframe to track against)
        TraceRange tr("mono track");
        PoseSeedArgs sa{};   // the start pose (dvo_batch_set_pose_guess_mode): k_mono_seed inside track()
        if (guess.on()) sa = guess.args(trk.state.as<SeqState>(), planned ? plan.eff.as<uint8_t>() : nullptr, DVO_SEQ_TRACK, xi_world.as<float>(), m);
        int rc = DVO_OK;
        trk.seed = guess.on() ? &sa : nullptr;
        trk.seed_mono = true;
        if (!planned) {
            rc = trk.track(frm, ref, stream);
        } else if (frame_id > 0) {
            TrackPlan tp = plan.track_plan(trk);
            tp.seq_k = trk.cam_k;
            rc = trk.track(frm, ref, stream, &tp);
        }
        trk.seed = nullptr;
        DVO_TRY(rc);
        guess.given.clear();
    }
    TraceRange tr_map("mono map (decide, propagate | update, promote, regularize)");
    DVO_HIP(hipMemsetAsync(need_list.p, 0, 4 * sizeof(int), stream));
    MonoPlanArgs ma{};
    if (planned) {
        ma.meta = m; ma.state = trk.state.as<SeqState>(); ma.eff = plan.eff.as<uint8_t>(); ma.started = started.as<uint8_t>();
        ma.need_save = need_save.as<int>(); ma.hist_xi = hist_xi.as<float>();
        ma.xi_world = xi_world.as<float>(); ma.T_world = T_world.as<float>(); ma.is_key = is_key.as<int>(); ma.need_list = need_list.as<int>();
        ma.n_seq = n_seq; ma.R = R; ma.max_frames = cfg.keyframe_max_frames; ma.min_translation = cfg.keyframe_min_translation;
        launch_mono_decide_plan(ma, stream);
    } else {
        launch_mono_decide(m, trk.state.as<SeqState>(), n_seq, frame_id, cfg.keyframe_min_translation, cfg.keyframe_max_frames,
                           xi_world.as<float>(), T_world.as<float>(), is_key.as<int>(), nullptr, stream, need_list.as<int>());
    }
    // ---- Mapper::estimate (mapper.cpp:16-33), both branches launched, each sequence takes its own ----
    {   // need: propagate the reference maps into the frame (mapper.cpp:62-74) ...
        PropArgs a{};
        a.ref_depth = ref.depth[T]; a.ref_sigma = ref.sigma[T]; a.ref_age = ref_age.as<float>();
        a.depth = frm.depth[T]; a.sigma = frm.sigma[T]; a.age = frm_age.as<float>();
        a.owner = owner.as<int>();
        a.w = tw; a.h = th; a.n_seq = n_seq; a.k = g.k[T]; a.meta = m;
        a.need_list = need_list.as<int>();
        a.seq_k = cam_top();   // (per-camera batch: k_propagate_owner_cam)
        if (pe) DVO_HIP(hipEventRecord(pe->e[0], stream));
        launch_propagate_batch(a, stream);
        if (pe) DVO_HIP(hipEventRecord(pe->e[1], stream));
    }
    DVO_TRY(queue_depth_update(frame_id, pe));   // !need: the stereo update of the reference maps (mapper.cpp:76-137)
    {   // ... need: the frame becomes the newest keyframe (FrameHistory::push, frame.hpp:151-157)
        PromoteArgs pa{};
        int sgi = 0;
        for (int l = 0; l < g.levels; l++) { pa.src[sgi] = frm.gray[l]; pa.dst[sgi] = ref.gray[l]; pa.count[sgi] = g.w[l] * g.h[l]; sgi++; }
        pa.src[sgi] = frm.depth[T]; pa.dst[sgi] = ref.depth[T]; pa.count[sgi] = np; sgi++;
        pa.src[sgi] = frm.sigma[T]; pa.dst[sgi] = ref.sigma[T]; pa.count[sgi] = np; sgi++;
        pa.src[sgi] = frm_age.as<float>(); pa.dst[sgi] = ref_age.as<float>(); pa.count[sgi] = np; sgi++;
        pa.n_seg = sgi; pa.n_seq = n_seq; pa.gray_top = frm.gray[T]; pa.ring_gray = ring_gray.as<float>(); pa.npix = np; pa.R = R;
        pa.meta = m;
        pa.need_list = need_list.as<int>();
        launch_promote(pa, stream);
        if (!planned) launch_mono_commit(m, hist_xi.as<float>(), n_seq, R, 0, frame_id, nullptr, nullptr, nullptr, stream);
    }
    // Mapper::regularize (mapper.cpp:139-144) of the newest keyframe, then Frame::updateDepthSigma / updateDepth (frame.cpp:39-61):
    // every level of depth and sigma is a decimation of the top maps, so ONE pass re-derives both pyramids (and the
    // weight) from the regularized depth and the current sigma -- the same values the reference's two re-decimations leave.
    {
        RegDecArgs ra{};
        ra.depth = ref.depth[T]; ra.sigma = ref.sigma[T];
        if (!depth_alt) depth_alt = tmp.as<float>();
        ra.depth_top_out = depth_alt;
        for (int l = 0; l < g.levels; l++) {
            ra.w[l] = g.w[l]; ra.h[l] = g.h[l];
            ra.depth_lv[l] = ref.depth[l]; ra.sigma_lv[l] = ref.sigma[l]; ra.wgt[l] = ref.wgt[l];
            ra.step[l] = ref.step[l];
        }
        ra.levels = g.levels; ra.n_seq = n_seq; ra.sigma_min = ref.sigma_min; ra.sigma_max = ref.sigma_max;
        if (pe) DVO_HIP(hipEventRecord(pe->e[4], stream));
        if (planned) {   // the TRACK sequences as above; SKIP copies its top-level depth forward; RESTART starts (k_regularize_redecimate_plan)
            MonoStartArgs sa{};
            sa.eff = plan.eff.as<uint8_t>(); sa.started = started.as<uint8_t>();
            sa.start_depth = start_depth; sa.start_sigma = start_sigma;
            sa.init_depth = init_depth.as<float>(); sa.init_sigma = init_sigma.as<float>();
            sa.sigma_top = ref.sigma[T]; sa.age = ref_age.as<float>();
            for (int l = 0; l < g.levels; l++) { sa.frm_gray[l] = frm.gray[l]; sa.ref_gray[l] = ref.gray[l]; }
            sa.ring_gray = ring_gray.as<float>(); sa.R = R;
            launch_regularize_redecimate_plan(ra, sa, stream);
        } else {
            launch_regularize_redecimate(ra, stream);
        }
        if (pe) { DVO_HIP(hipEventRecord(pe->e[5], stream)); map_ev_used++; }
        std::swap(ref.depth[T], depth_alt);   // the top-level depth map alternates between the arena block and `tmp`
    }
    if (planned) {   // FrameHistory::push of the TRACK keyframes, frame 0 of the RESTART sequences, the SKIP need flags back
        launch_mono_commit_plan(ma, stream);
        plan.consumed();
        start_depth = start_sigma = nullptr;
    }
    DVO_HIP(hipGetLastError());
    quality.ready = quality.on;
    trk.end_terms(stream);
    latest_id = frame_id;
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ mono: per-sequence actions
int MonoBatch::alloc_plan()
{
    if (need_save.p) return DVO_OK;
    const size_t n = (size_t)n_seq;
    DVO_TRY(plan.alloc(n_seq, trk.n_sub, latest_id >= 0, stream));   // (after plain calls every sequence has a keyframe)
    DVO_TRY(started.alloc(n));
    DVO_TRY(need_save.alloc(sizeof(int) * n));
    DVO_HIP(hipMemsetAsync(started.p, latest_id >= 0 ? 1 : 0, n, stream));
    if (!host_init) {   // the start map of a later start without a host map: the default (what dvo_vo uses)
        std::vector<float> d, s;
        const size_t np = (size_t)top_pixels();
        default_initial_depth((int)np, cfg.rng_seed, d, s);
        DVO_HIP(hipMemcpy(init_depth.p, d.data(), np * sizeof(float), hipMemcpyHostToDevice));
        DVO_HIP(hipMemcpy(init_sigma.p, s.data(), np * sizeof(float), hipMemcpyHostToDevice));
    }
    return DVO_OK;
}

int MonoBatch::set_actions(const uint8_t* actions, bool on_device)
{
    if (actions) {
        DVO_TRY(select_device(device));
        DVO_TRY(alloc_plan());
    }
    return plan.set_actions(actions, on_device, n_seq, stream);
}

int MonoBatch::set_start_depth(const float* depth_dev, const float* sigma_dev)
{
    if (!depth_dev != !sigma_dev) { set_error("dvo_batch_set_mono_start_depth_device: depth and sigma are both set or both NULL"); return DVO_ERR_BAD_ARGUMENT; }
    if (depth_dev) {
        DVO_TRY(select_device(device));
        DVO_TRY(alloc_plan());
    }
    start_depth = depth_dev; start_sigma = sigma_dev;
    return DVO_OK;
}

int MonoBatch::status_of_last(int* out, bool out_on_device)
{
    if (latest_id < 0) { set_error("dvo_batch_mono_last_status: no frame has been consumed yet"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    return plan.status_of_last(out, out_on_device, n_seq, latest_id == 0, stream);
}

int MonoBatch::set_guess_mode(int mode)
{
    DVO_TRY(select_device(device));
    // the call before: its effective actions (per-sequence path), else all STARTED (first call) or all TRACKED (later ones)
    const uint8_t* pe = plan.act_used ? plan.eff.as<uint8_t>() : nullptr;
    const int all = latest_id < 0 ? 0xff : (latest_id == 0 ? DVO_SEQ_RESTART : DVO_SEQ_TRACK);
    return guess.set_mode(mode, n_seq, stream, pe, all);
}

int MonoBatch::started_of(int seq, bool* out)
{
    if (latest_id < 0) { *out = false; return DVO_OK; }
    if (!plan.act_used) { *out = true; return DVO_OK; }
    uint8_t v = 0;
    DVO_HIP(hipMemcpyAsync(&v, started.as<uint8_t>() + seq, 1, hipMemcpyDeviceToHost, stream));
    DVO_HIP(hipStreamSynchronize(stream));
    *out = v != 0;
    return DVO_OK;
}

// the keyframes of a mono batch (dvo_batch_export_points): `ref`, its age map, `meta`; `started` once actions have been used
PointsExport::Source MonoBatch::points_source(int level) const
{
    PointsExport::Source src;
    src.meta = meta.as<MonoSeq>(); src.is_key = is_key.as<int>();
    src.started = plan.act_used ? started.as<uint8_t>() : nullptr;   // (plain calls: every sequence has a keyframe)
    src.depth = ref.depth[level]; src.gray = ref.gray[level]; src.sigma = ref.sigma[level];
    src.age = level == g.top() ? ref_age.as<float>() : nullptr;
    src.seq_k = cam_dev.p ? cam_dev.as<Intr>() + (size_t)level * n_seq : nullptr;
    src.k = g.k[level];
    src.w = g.w[level]; src.h = g.h[level]; src.top_w = g.w[g.top()]; src.top_h = g.h[g.top()]; src.n_seq = n_seq;
    return src;
}

}  // namespace dvo

using namespace dvo;

extern "C" {

static int create_mono(int n_seq, const float* K, bool per_camera, int width, int height, int ring_keyframes, const dvo_config* cfg, dvo_batch** out)
{
    if (!out) return DVO_ERR_BAD_ARGUMENT;
    *out = nullptr;
    dvo_batch* b = new (std::nothrow) dvo_batch();
    if (!b) return DVO_ERR_OUT_OF_MEMORY;
    b->mono.reset(new (std::nothrow) MonoBatch());
    if (!b->mono) { delete b; return DVO_ERR_OUT_OF_MEMORY; }
    const int st = b->mono->init(n_seq, K, width, height, ring_keyframes > 0 ? ring_keyframes : 8, cfg, per_camera);
    if (st != DVO_OK) { delete b; return st; }
    *out = b;
    return DVO_OK;
}

int dvo_batch_create_mono(int n_seq, const float K[9], int width, int height, int ring_keyframes, const dvo_config* cfg, dvo_batch** out)
{
    return create_mono(n_seq, K, false, width, height, ring_keyframes, cfg, out);
}

int dvo_batch_create_mono_cameras(int n_seq, const float* K, int width, int height, int ring_keyframes, const dvo_config* cfg, dvo_batch** out)
{
    return create_mono(n_seq, K, true, width, height, ring_keyframes, cfg, out);
}

#define DVO_NEED_MONO(b)                                                                                      \
    do {                                                                                                      \
        if (!(b) || !(b)->mono) { set_error("this entry point needs a mono batch (dvo_batch_create_mono)"); return DVO_ERR_BAD_ARGUMENT; } \
    } while (0)

int dvo_batch_set_initial_depth(dvo_batch* b, const float* depth, const float* sigma)
{
    DVO_NEED_MONO(b);
    return b->mono->set_initial_depth(depth, sigma);
}

int dvo_batch_set_initial_depth_device(dvo_batch* b, const float* depth_dev, const float* sigma_dev)
{
    DVO_NEED_MONO(b);
    return b->mono->set_initial_depth_device(depth_dev, sigma_dev);
}

int dvo_batch_odometrize_device(dvo_batch* b, const float* gray_dev)
{
    DVO_NEED_MONO(b);
    FrameInput in;
    in.gray = gray_dev;
    return b->mono->odometrize(in);
}

int dvo_batch_odometrize_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels)
{
    DVO_NEED_MONO(b);
    FrameInput in;
    in.rgb = rgb_dev; in.channels = channels;
    return b->mono->odometrize(in);
}

int dvo_batch_odometrize_host(dvo_batch* b, const float* gray)
{
    DVO_NEED_MONO(b);
    FrameInput in;
    in.gray = gray;
    return b->mono->odometrize_host(gray, in);
}

int dvo_batch_odometrize_raw_host(dvo_batch* b, const uint8_t* rgb, int channels)
{
    DVO_NEED_MONO(b);
    if (channels != 1 && channels != 3 && channels != 4) { set_error("bad channel count"); return DVO_ERR_BAD_ARGUMENT; }
    FrameInput in;
    in.rgb = rgb; in.channels = channels;
    return b->mono->odometrize_host(rgb, in);
}

int dvo_batch_set_distortion(dvo_batch* b, const float* D, int per_sequence)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (!b->mono) { set_error("dvo_batch_set_distortion: needs a mono batch (sensor-depth batches do not undistort)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->mono->set_distortion(D, per_sequence != 0);
}

int dvo_batch_set_photometric(dvo_batch* b, int n_cal, const float* inv_response, const float* vignette, const int* seq_cal)
{
    if (!b) { set_error("dvo_batch_set_photometric: null handle"); return DVO_ERR_BAD_ARGUMENT; }
    if (!b->mono) { set_error("dvo_batch_set_photometric: needs a mono batch (sensor-depth batches are not calibrated)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->mono->set_photometric(n_cal, inv_response, vignette, seq_cal);
}

int dvo_batch_get_photometric(dvo_batch* b, int* n_cal, int* seq_cal)
{
    DVO_NEED_MONO(b);
    const MonoBatch& M = *b->mono;
    if (n_cal) *n_cal = M.pho.n_cal;
    if (seq_cal) {
        if (M.pho.enabled()) memcpy(seq_cal, M.pho.seq_cal.data(), sizeof(int) * (size_t)M.n_seq);
        else memset(seq_cal, 0, sizeof(int) * (size_t)M.n_seq);
    }
    return DVO_OK;
}

int dvo_debug_batch_photometric_gain(dvo_batch* b, int seq, float* gain)
{
    DVO_NEED_MONO(b);
    MonoBatch& M = *b->mono;
    if (!gain || seq < 0 || seq >= M.n_seq) { set_error("dvo_debug_batch_photometric_gain: null output or sequence out of range"); return DVO_ERR_BAD_ARGUMENT; }
    if (!M.pho.enabled()) { set_error("dvo_debug_batch_photometric_gain: the batch has no photometric calibration"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(M.device));
    const size_t np = (size_t)M.top_pixels();
    DVO_HIP(hipMemcpyAsync(gain, M.pho.gain_dev.as<float>() + np * (size_t)M.pho.seq_pair[(size_t)seq], np * sizeof(float), hipMemcpyDeviceToHost, M.stream));
    DVO_HIP(hipStreamSynchronize(M.stream));
    return DVO_OK;
}

int dvo_debug_batch_last_pyramid_kernel(dvo_batch* b, dvo_pyramid_kernel* ran)
{
    DVO_NEED_MONO(b);
    if (!ran) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono->latest_id < 0) return DVO_ERR_NOT_READY;
    ran->kind = b->mono->last_build.kind; ran->culls = b->mono->last_build.culls; ran->plan = b->mono->last_build.plan;
    return DVO_OK;
}

int dvo_batch_get_distortion(dvo_batch* b, float* D, int* enabled)
{
    DVO_NEED_MONO(b);
    const MonoBatch& M = *b->mono;
    if (D) {
        if (M.und.enabled()) memcpy(D, M.und.D.data(), sizeof(float) * M.und.D.size());
        else memset(D, 0, sizeof(float) * 5 * (size_t)M.n_seq);
    }
    if (enabled) *enabled = M.und.enabled() ? 1 : 0;
    return DVO_OK;
}

// The world poses of a batch: a mono batch's, or a sensor-depth batch's with keyframe tracking (dvo_batch_set_keyframe_tracking).  A plain
// sensor-depth batch has none.
namespace {
struct WorldPoses {
    const void* xi; const void* T; const void* key;
    size_t n; hipStream_t s; int device; bool ready;
};
}  // namespace
static int world_poses_of(dvo_batch* b, WorldPoses& w)
{
    if (b && b->mono) {
        const MonoBatch& M = *b->mono;
        w = {M.xi_world.p, M.T_world.p, M.is_key.p, (size_t)M.n_seq, M.stream, M.device, M.latest_id >= 0};
        return DVO_OK;
    }
    if (b && b->impl.kf_on) {
        const Batch& B = b->impl;
        w = {B.xi_world.p, B.T_world.p, B.is_key.p, (size_t)B.n_seq, B.stream, B.device, B.n_push > 0};
        return DVO_OK;
    }
    set_error("this entry point needs a mono batch (dvo_batch_create_mono) or a sensor-depth batch with keyframe tracking (dvo_batch_set_keyframe_tracking)");
    return DVO_ERR_BAD_ARGUMENT;
}

int dvo_batch_world_poses(dvo_batch* b, float* xi_world, float* T_world, int* is_keyframe)
{
    WorldPoses w;
    DVO_TRY(world_poses_of(b, w));
    if (!w.ready) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(w.device));
    if (xi_world) DVO_HIP(hipMemcpyAsync(xi_world, w.xi, sizeof(float) * 6 * w.n, hipMemcpyDeviceToHost, w.s));
    if (T_world) DVO_HIP(hipMemcpyAsync(T_world, w.T, sizeof(float) * 16 * w.n, hipMemcpyDeviceToHost, w.s));
    if (is_keyframe) DVO_HIP(hipMemcpyAsync(is_keyframe, w.key, sizeof(int) * w.n, hipMemcpyDeviceToHost, w.s));
    DVO_HIP(hipStreamSynchronize(w.s));
    return DVO_OK;
}

int dvo_batch_copy_world_poses_device(dvo_batch* b, float* xi_dst_dev, float* T_dst_dev, int* key_dst_dev)
{
    WorldPoses w;
    DVO_TRY(world_poses_of(b, w));
    if (!w.ready) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(w.device));
    if (xi_dst_dev) DVO_HIP(hipMemcpyAsync(xi_dst_dev, w.xi, sizeof(float) * 6 * w.n, hipMemcpyDeviceToDevice, w.s));
    if (T_dst_dev) DVO_HIP(hipMemcpyAsync(T_dst_dev, w.T, sizeof(float) * 16 * w.n, hipMemcpyDeviceToDevice, w.s));
    if (key_dst_dev) DVO_HIP(hipMemcpyAsync(key_dst_dev, w.key, sizeof(int) * w.n, hipMemcpyDeviceToDevice, w.s));
    return DVO_OK;
}

// ---- keyframe maps as compacted world-frame point clouds -----------------------------------------------------------
void dvo_points_config_default(dvo_points_config* cfg)
{
    if (!cfg) return;
    cfg->struct_size = (int)sizeof(dvo_points_config);
    cfg->select = DVO_POINTS_ALL;
    cfg->level = -1;           // the top level
    cfg->stride = 1;
    cfg->min_depth = -1.0f;    // the handle's dvo_config::min_depth
    cfg->max_depth = __builtin_inff();
    cfg->max_sigma = __builtin_inff();
    cfg->min_age = 0.0f;
    cfg->min_count = 0;
}

int dvo_batch_export_points(dvo_batch* b, const dvo_points_config* cfg, uint32_t capacity, float* xyzg_dev, uint32_t* src_dev, float* sigma_dev,
                            uint32_t* offsets_dev)
{
    static const char who[] = "dvo_batch_export_points";
    const auto bad = [](const char* what) { set_error(std::string(who) + ": " + what); return DVO_ERR_BAD_ARGUMENT; };
    if (!b || !cfg || !offsets_dev) return DVO_ERR_BAD_ARGUMENT;
    WorldPoses wp;
    DVO_TRY(world_poses_of(b, wp));   // a mono batch, or a sensor-depth batch with keyframe tracking
    const bool mono = b->mono != nullptr;
    const Geometry& g = mono ? b->mono->g : b->impl.g;
    const float inf = __builtin_inff();
    if (cfg->struct_size != (int)sizeof(dvo_points_config)) return bad("struct_size is not sizeof(dvo_points_config)");
    if (cfg->select != DVO_POINTS_ALL && cfg->select != DVO_POINTS_NEW) return bad("select is DVO_POINTS_ALL or DVO_POINTS_NEW");
    if (cfg->level < -1 || cfg->level >= g.levels) return bad("level is outside [0, levels) (-1: the top level)");
    if (cfg->stride < 1) return bad("stride must be >= 1");
    dvo_points_config c = *cfg;
    if (c.level < 0) c.level = g.top();
    if (!(fabsf(c.min_depth) < inf)) return bad("min_depth must be finite");
    if (c.min_depth < 0.0f) c.min_depth = mono ? b->mono->cfg.min_depth : b->impl.cfg.min_depth;
    if (!(c.max_depth >= c.min_depth)) return bad("max_depth must be >= min_depth");
    if (c.max_sigma != c.max_sigma) return bad("max_sigma must not be NaN");
    const bool top = c.level == g.top();
    if (!mono && (c.max_sigma != inf || sigma_dev)) return bad("a sensor-depth batch stores no sigma maps of its keyframes (max_sigma = +inf, sigma_dev = NULL)");
    if (!(c.min_age >= 0.0f && c.min_age < inf)) return bad("min_age must be finite and >= 0");
    if (c.min_age != 0.0f && !(mono && top)) return bad("min_age applies to the top level of a mono batch only");
    if (c.min_count < 0 || c.min_count > 255) return bad("min_count is outside [0, 255]");
    if (c.min_count != 0 && !(!mono && top && b->impl.fuse.ran)) return bad("min_count applies to the top level of a sensor-depth batch that has fused (dvo_batch_set_keyframe_fusion) only");
    if (capacity > 0x7fffffffu) return bad("capacity is above 2^31 - 1");
    if (capacity > 0 && (!xyzg_dev || (reinterpret_cast<uintptr_t>(xyzg_dev) & 15u))) return bad("xyzg_dev must be a 16-byte aligned device buffer when capacity > 0");
    const long long plane = (long long)g.w[c.level] * g.h[c.level];
    if (plane > DVO_POINTS_MAX_PLANE) return bad("the level has more than 2^24 pixels");
    if (plane * (long long)wp.n > 0x7fffffffLL) return bad("n_seq * w_l * h_l is above 2^31 - 1");
    if (!wp.ready) return DVO_ERR_NOT_READY;
    if (!mono && b->impl.cam_pending) {
        set_error(std::string(who) + ": the per-sequence intrinsics changed since the last push (the keyframes belong to that push's cameras): export before dvo_batch_set_intrinsics or after the next push");
        return DVO_ERR_NOT_READY;
    }
    DVO_TRY(select_device(wp.device));
    if (capacity == 0) { xyzg_dev = nullptr; src_dev = nullptr; sigma_dev = nullptr; }
    if (mono) return b->mono->points.run(b->mono->points_source(c.level), c, capacity, xyzg_dev, src_dev, sigma_dev, offsets_dev, wp.s);
    return b->impl.points.run(b->impl.points_source(c.level), c, capacity, xyzg_dev, src_dev, sigma_dev, offsets_dev, wp.s);
}

int dvo_batch_last_points(dvo_batch* b, uint32_t* offsets)
{
    if (!b || !offsets) return DVO_ERR_BAD_ARGUMENT;
    WorldPoses wp;
    DVO_TRY(world_poses_of(b, wp));
    const PointsExport& P = b->mono ? b->mono->points : b->impl.points;
    if (!P.ready) { set_error("dvo_batch_last_points: no dvo_batch_export_points call yet"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(wp.device));
    DVO_HIP(hipMemcpyAsync(offsets, P.offsets.p, sizeof(uint32_t) * (wp.n + 1), hipMemcpyDeviceToHost, wp.s));
    DVO_HIP(hipStreamSynchronize(wp.s));
    return DVO_OK;
}

// the keyframe of a sensor-depth batch with keyframe tracking: gray / depth of one level of the keyframe set, its twist, id and count
static int sensor_keyframe_get(Batch& B, int seq, int level, float* gray, float* depth, float* sigma, float* age, float xi[6], int* id,
                               int* n_keyframes, int* valid_updates)
{
    if (seq < 0 || seq >= B.n_seq || level < 0 || level >= B.g.levels) return DVO_ERR_BAD_ARGUMENT;
    if (sigma || age) {
        set_error("dvo_batch_keyframe_get: a sensor-depth batch stores no sigma or age maps of its keyframes (pass NULL)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (B.n_push == 0) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(B.device));
    MonoSeq m;
    DVO_HIP(hipMemcpyAsync(&m, B.kf_meta.as<MonoSeq>() + seq, sizeof m, hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    if (m.n_total == 0) { set_error("dvo_batch_keyframe_get: the sequence has not started (it was skipped on every push so far)"); return DVO_ERR_NOT_READY; }
    const size_t n = (size_t)B.g.w[level] * B.g.h[level], off = n * (size_t)seq;
    if (gray) DVO_HIP(hipMemcpyAsync(gray, B.fs[B.cur].gray[level] + off, n * 4, hipMemcpyDeviceToHost, B.stream));
    if (depth) DVO_HIP(hipMemcpyAsync(depth, B.fs[B.cur].depth[level] + off, n * 4, hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    if (xi) memcpy(xi, m.ref_xi, 6 * sizeof(float));
    if (id) *id = m.ref_id;
    if (n_keyframes) *n_keyframes = m.n_total;
    if (valid_updates) *valid_updates = 0;
    return DVO_OK;
}

int dvo_batch_keyframe_get(dvo_batch* b, int seq, int level, float* gray, float* depth, float* sigma, float* age, float xi[6], int* id,
                           int* n_keyframes, int* valid_updates)
{
    if (b && !b->mono && b->impl.kf_on) return sensor_keyframe_get(b->impl, seq, level, gray, depth, sigma, age, xi, id, n_keyframes, valid_updates);
    DVO_NEED_MONO(b);
    MonoBatch& M = *b->mono;
    if (seq < 0 || seq >= M.n_seq || level < 0 || level >= M.g.levels) return DVO_ERR_BAD_ARGUMENT;
    if (M.latest_id < 0) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(M.device));
    bool st = false;
    DVO_TRY(M.started_of(seq, &st));
    if (!st) { set_error("dvo_batch_keyframe_get: the sequence has not started (it was skipped on every call so far)"); return DVO_ERR_NOT_READY; }
    hipStream_t s = M.stream;
    const size_t n = (size_t)M.g.w[level] * M.g.h[level], off = n * (size_t)seq;
    if (gray) DVO_HIP(hipMemcpyAsync(gray, M.ref.gray[level] + off, n * 4, hipMemcpyDeviceToHost, s));
    if (depth) DVO_HIP(hipMemcpyAsync(depth, M.ref.depth[level] + off, n * 4, hipMemcpyDeviceToHost, s));
    if (sigma) DVO_HIP(hipMemcpyAsync(sigma, M.ref.sigma[level] + off, n * 4, hipMemcpyDeviceToHost, s));
    if (age) {
        if (level != M.g.top()) { set_error("age is stored for the top level only"); return DVO_ERR_BAD_ARGUMENT; }
        DVO_HIP(hipMemcpyAsync(age, M.ref_age.as<float>() + off, n * 4, hipMemcpyDeviceToHost, s));
    }
    MonoSeq m;
    DVO_HIP(hipMemcpyAsync(&m, M.meta.as<MonoSeq>() + seq, sizeof m, hipMemcpyDeviceToHost, s));
    DVO_HIP(hipStreamSynchronize(s));
    if (xi) memcpy(xi, m.ref_xi, 6 * sizeof(float));
    if (id) *id = m.ref_id;
    if (n_keyframes) *n_keyframes = m.n_total;
    if (valid_updates) *valid_updates = m.valid_updates;
    return DVO_OK;
}

int dvo_batch_mono_stats(dvo_batch* b, int seq, dvo_mono_stats* out)
{
    DVO_NEED_MONO(b);
    MonoBatch& M = *b->mono;
    if (!out || seq < 0 || seq >= M.n_seq) return DVO_ERR_BAD_ARGUMENT;
    if (M.latest_id < 0) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(M.device));
    bool st = false;
    DVO_TRY(M.started_of(seq, &st));
    if (!st) { set_error("dvo_batch_mono_stats: the sequence has not started (it was skipped on every call so far)"); return DVO_ERR_NOT_READY; }
    MonoSeq m;
    DVO_HIP(hipMemcpyAsync(&m, M.meta.as<MonoSeq>() + seq, sizeof m, hipMemcpyDeviceToHost, M.stream));
    DVO_HIP(hipStreamSynchronize(M.stream));
    out->frames = M.plan.act_used ? m.frame_id + 1 : M.latest_id + 1;   // (with actions: the frames since the sequence's last start)
    out->keyframes_created = m.n_total;
    out->ring_keyframes = M.R;
    out->valid_updates_last_frame = m.valid_updates;
    out->clamped_pixels = m.clamped;
    return DVO_OK;
}

int dvo_batch_set_mono_actions(dvo_batch* b, const uint8_t* actions, int actions_on_device)
{
    DVO_NEED_MONO(b);
    return b->mono->set_actions(actions, actions_on_device != 0);
}

int dvo_batch_mono_last_status(dvo_batch* b, int* status)
{
    DVO_NEED_MONO(b);
    if (!status) return DVO_ERR_BAD_ARGUMENT;
    return b->mono->status_of_last(status, false);
}

int dvo_batch_copy_mono_status_device(dvo_batch* b, int* status_dev)
{
    DVO_NEED_MONO(b);
    if (!status_dev) return DVO_ERR_BAD_ARGUMENT;
    return b->mono->status_of_last(status_dev, true);
}

int dvo_batch_set_mono_start_depth_device(dvo_batch* b, const float* depth_dev, const float* sigma_dev)
{
    DVO_NEED_MONO(b);
    return b->mono->set_start_depth(depth_dev, sigma_dev);
}

int dvo_batch_profile_mapping(dvo_batch* b, dvo_map_profile* out, int reset)
{
    DVO_NEED_MONO(b);
    MonoBatch& M = *b->mono;
    if (!out) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(M.device));
    DVO_TRY(M.collect_map_profile());
    out->frames = M.prof_frames;
    out->depth_update_ms = M.prof_update_ms;
    out->regularize_ms = M.prof_regularize_ms;
    out->propagate_ms = M.prof_propagate_ms;
    const int T = M.g.top(), w = M.g.w[T], h = M.g.h[T];
    // the window of mapper.cpp:90 (cols 16..144, rows 12..108 at 160x120) when crop_enable, else the whole map
    const int cx = M.cfg.crop_enable ? ((w - 1 < 144 ? w - 1 : 144) - 16 + 1) : w, cy = M.cfg.crop_enable ? ((h - 1 < 108 ? h - 1 : 108) - 12 + 1) : h;
    const int wx = cx > 0 ? cx : 0, wy = cy > 0 ? cy : 0;   // (as launch_depth_update)
    out->update_window_pixels = (uint64_t)wx * wy * (uint64_t)M.n_seq;
    out->map_pixels = (uint64_t)w * h * (uint64_t)M.n_seq;
    if (reset) { M.prof_frames = 0; M.prof_update_ms = M.prof_regularize_ms = M.prof_propagate_ms = 0; }
    return DVO_OK;
}

}  // extern "C"
