// coeb_ctx.hpp -- the context behind the C-ABI's coeb_ctx handle and the host helpers every
// .hip file's entry points share (defined in coeb_capi.hip).  The plan the context caches per
// image size is built by coeb_plan.cpp.  Host code only.
#pragma once
#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/coeb_front.h"
#include "coeb_internal.hpp"
#include "coeb_plan.hpp"
#include "coeb_voc.hpp"

// One device allocation of a context, grown by ensure(); `name` is the text of its COEB_ENOMEM message.
template <class T>
struct DevArr {
    const char* name;
    T* p = nullptr;
    size_t bytes = 0;
};

// The context's device buffers, grouped by the stage that owns them.  all() lists every field of
// its group once (each_buf checks the count): coeb_destroy frees by walking it.
struct PlanBufs {           // ensure_plan
    DevArr<Plan> plan{"plan"};
    DevArr<int> rtab{"rtab"};     // resize tables and row descriptors (make_plan)
    DevArr<CellDesc> cells{"cells"};
    DevArr<int8_t> pattern{"pattern"};
    auto all() { return std::tie(plan, rtab, cells, pattern); }
};
struct ExtractDev {         // extract_bufs / upload_dyn and the host-buffer staging (layout: coeb_internal.hpp)
    DevArr<uint8_t> pyr{"pyr"}, blur{"blur"}, nodes{"nodes"}, desc{"desc"}, gray_stage{"gray_stage"}, stage{"stage"};
    DevArr<int> cand_n{"cand_n"}, lvl_n{"lvl_n"}, counts{"counts"}, err{"err"};
    DevArr<uint32_t> cand{"cand"}, keys{"keys"}, lvl_kp{"lvl_kp"};
    DevArr<coeb_keypoint> kps{"kps"};
    DevArr<DynMask> dyn{"dyn"};
    DevArr<float> boxes{"boxes"}, tm{"tm"};
    DevArr<int32_t> box_off{"box_off"}, blurf{"blurf"}, tm_off{"tm_off"};
    auto all()
    {
        return std::tie(pyr, blur, nodes, desc, gray_stage, stage, cand_n, lvl_n, counts, err, cand, keys, lvl_kp, kps, dyn,
                        boxes, tm, box_off, blurf, tm_off);
    }
};
struct FrameBatchBufs {     // coeb_frame_batch_device
    DevArr<float> f_tm{"f_tm"};
    DevArr<int32_t> f_ntm{"f_ntm"}, f_bframe{"f_bframe"}, f_blur{"f_blur"};
    auto all() { return std::tie(f_tm, f_ntm, f_bframe, f_blur); }
};
struct BatchMatchBufs {     // coeb_match_batch_device*
    DevArr<float> b_ur{"b_ur"}, b_dep{"b_dep"}, b_xw{"b_xw"}, b_I{"b_I"}, b_T{"b_T"};
    DevArr<uint8_t> b_has{"b_has"}, b_outl{"b_outl"};
    DevArr<int32_t> b_mqn{"b_mqn"}, b_nobs{"b_nobs"}, b_match{"b_match"}, b_nm{"b_nm"}, b_scr{"b_scr"};
    auto all() { return std::tie(b_ur, b_dep, b_xw, b_I, b_T, b_has, b_outl, b_mqn, b_nobs, b_match, b_nm, b_scr); }
};
struct BatchPoseBufs {      // coeb_pose_batch_device (k_pose's own snapshots)
    DevArr<float> t_T{"t_T"}, t_xw{"t_xw"}, t_isg{"t_isg"}, t_ur{"t_ur"};
    DevArr<uint8_t> t_has{"t_has"}, t_outl{"t_outl"}, t_act{"t_act"};
    DevArr<int32_t> t_n{"t_n"}, t_res{"t_res"};
    DevArr<PoseEdgeRec> t_edge{"t_edge"};
    DevArr<double> t_chi{"t_chi"};
    DevArr<coeb_keypoint> t_kp{"t_kp"};
    auto all() { return std::tie(t_T, t_xw, t_isg, t_ur, t_has, t_outl, t_act, t_n, t_res, t_edge, t_chi, t_kp); }
};
struct TrackLocalMapBufs {  // coeb_track_local_map_batch_device
    DevArr<uint8_t> tl_sdesc{"tl_sdesc"}, tl_shas{"tl_shas"}, tl_seen{"tl_seen"}, tl_active{"tl_active"},
        tl_inview{"tl_inview"}, tl_has2{"tl_has2"}, tl_outl2{"tl_outl2"};
    DevArr<int8_t> tl_soct{"tl_soct"};
    DevArr<float> tl_sxw{"tl_sxw"}, tl_px{"tl_px"}, tl_py{"tl_py"}, tl_pxr{"tl_pxr"}, tl_vcos{"tl_vcos"}, tl_lxw{"tl_lxw"},
        tl_xw2{"tl_xw2"}, tl_T2{"tl_T2"};
    DevArr<int32_t> tl_sm1{"tl_sm1"}, tl_scnt{"tl_scnt"}, tl_snm1{"tl_snm1"}, tl_cobs{"tl_cobs"}, tl_nmap{"tl_nmap"},
        tl_level{"tl_level"}, tl_lnobs{"tl_lnobs"}, tl_lmatch{"tl_lmatch"}, tl_nlocal{"tl_nlocal"}, tl_path{"tl_path"},
        tl_n2{"tl_n2"}, tl_res2{"tl_res2"};
    DevArr<uint32_t> tl_lists{"tl_lists"};
    auto all()
    {
        return std::tie(tl_sdesc, tl_shas, tl_seen, tl_active, tl_inview, tl_has2, tl_outl2, tl_soct, tl_sxw, tl_px, tl_py,
                        tl_pxr, tl_vcos, tl_lxw, tl_xw2, tl_T2, tl_sm1, tl_scnt, tl_snm1, tl_cobs, tl_nmap, tl_level,
                        tl_lnobs, tl_lmatch, tl_nlocal, tl_path, tl_n2, tl_res2, tl_lists);
    }
};
struct SingleFrameBufs {    // scratch only (results live in the call's staged region): coeb_match_lastframe (m_*),
                            // _localmap / _keyframe (l_*), coeb_pose_optimization (p_*);
                            // coeb_search_local_points / coeb_track_local_map use l_list, l_path and p_*
                            // coeb_track_reference_keyframe uses p_* (and BowBufs' m_csr / m_aux)
    DevArr<int32_t> m_scr{"m_scr"}, m_qn{"m_qn"}, l_path{"l_path"};
    DevArr<uint32_t> l_list{"l_list"};
    DevArr<uint8_t> p_act{"p_act"};
    DevArr<PoseEdgeRec> p_edge{"p_edge"};
    DevArr<double> p_chi{"p_chi"};
    auto all() { return std::tie(m_scr, m_qn, l_path, l_list, p_act, p_edge, p_chi); }
};
struct TimingBufs {         // diagnostic phase clocks (COEB_MATCH_CLOCK / COEB_POSE_CLOCK builds)
    DevArr<long long> m_timing{"m_timing"}, p_timing{"p_timing"};
    auto all() { return std::tie(m_timing, p_timing); }
};
struct HelperBufs {         // scratch of coeb_flow.hip (flow) and of coeb_frame.hip's host-buffer entry points
    DevArr<uint8_t> flow{"flow"}, bf_img{"bf_img"}, pp_img{"pp_img"}, pp_gray{"pp_gray"}, pp_dsrc{"pp_dsrc"};
    DevArr<float> bf_box{"bf_box"}, pp_dep{"pp_dep"};
    DevArr<int32_t> bf_out{"bf_out"};
    DevArr<coeb_keypoint> ud_in{"ud_in"}, ud_out{"ud_out"};
    auto all() { return std::tie(flow, bf_img, pp_img, pp_gray, pp_dsrc, bf_box, pp_dep, bf_out, ud_in, ud_out); }
};
struct BowBufs {            // coeb_bow.hip: the vocabulary tables (v_*), the batch transform's ids (b_*) and the
                            // scratch SearchByBoW's callers share (m_csr, m_aux; coeb_kfdb.hip too)
    DevArr<VocRec> v_rec{"v_rec"};
    DevArr<uint8_t> v_desc{"v_desc"};
    DevArr<int32_t> b_word{"b_word"}, b_node{"b_node"}, m_csr{"m_csr"}, m_aux{"m_aux"};
    auto all() { return std::tie(v_rec, v_desc, b_word, b_node, m_csr, m_aux); }
};

template <class G, class F>
void each_buf(G& g, F f)
{
    auto t = g.all();
    static_assert(std::tuple_size<decltype(t)>::value * sizeof(DevArr<char>) == sizeof(G), "all() must list every buffer");
    std::apply([&](auto&... a) { (f(a), ...); }, t);
}

struct ProfImpl {
    bool enabled = false;
    std::vector<std::string> names;
    std::vector<double> ms;
    std::vector<int64_t> launches;
    std::vector<hipEvent_t> pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
    int cur_name = -1;
    hipEvent_t cur_start = nullptr;
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    void drain()
    {
        for (auto& pe : pending) {
            float t = 0.f;
            (void)hipEventSynchronize(pe.second.second);
            (void)hipEventElapsedTime(&t, pe.second.first, pe.second.second);
            ms[pe.first] += t;
            launches[pe.first] += 1;
            pool.push_back(pe.second.first);
            pool.push_back(pe.second.second);
        }
        pending.clear();
    }
};

struct coeb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    coeb_orb_params params{};
    Tables tab{};
    int max_w = 0, max_h = 0, max_batch = 0;
    bool has_plan = false;
    Plan plan{};
    std::vector<int> rtab;
    std::vector<CellDesc> cells;
    PlanBufs pl;
    ExtractDev ex;
    FrameBatchBufs fb;
    BatchMatchBufs bm;
    BatchPoseBufs bp;
    TrackLocalMapBufs tl;
    SingleFrameBufs sf;
    TimingBufs tim;
    HelperBufs hl;
    BowBufs bow;
    // the vocabulary of coeb_bow_set_vocabulary (k == 0: none): shape, and the word weights the
    // single-frame transform gathers on the host
    struct { int k = 0, L = 0, nnodes = 0; std::vector<double> word_weight; } voc;
    int bow_frames = 0;        // frames of the last coeb_bow_batch_device
    std::vector<coeb_kfdb*> kfdbs;     // the keyframe databases alive on this context (coeb_kfdb.hip)
    std::string err;
    ProfImpl prof;
    ProfileHook hook;
    int batch_frames = 0;      // frames of the last extracted batch
    const uint8_t* batch_gray = nullptr;
    int ident_frames = 0;      // identity poses initialised in bm.b_I
    // Batch chunking over several HIP streams (coeb_set_batch_streams): chunk k = frames
    // [chunk[k], chunk[k+1]) runs extract -> prep -> match on subs[k]; match of chunk k's first
    // frame waits for chunk k-1's prep (its LastFrame).  The context stream joins the chunk
    // streams lazily, before anything else is enqueued on it (main_stream()).
    int nstreams = 1;
    std::vector<hipStream_t> subs;
    std::vector<int> chunk;                      // chunk boundaries of the last batch
    std::vector<hipEvent_t> ev_prep, ev_mdone;   // per chunk: prep done / match done
    bool mdone_valid = false;                    // ev_mdone holds the previous batch's matches
    bool pending_join = false;
    bool extract_chunked = false;                // the last batch extract ran on the chunk streams
    hipEvent_t ev_main = nullptr, ev_join = nullptr;
    // coeb_pose_batch_device runs k_pose on its own stream, so the optimiser of batch k overlaps
    // the extraction and matching of batch k+1 (k_pose is latency bound, one workgroup per frame;
    // the extraction kernels are VALU bound).  k_track_prep copies everything k_pose reads into
    // t_* buffers; the next coeb_pose_batch_device, coeb_batch_pose_results, coeb_memcpy_d2h,
    // coeb_synchronize and coeb_destroy join it (join_pose()).
    hipStream_t pose_stream = nullptr;
    // level-0 blur + FAST beside the pyramid (launch_extract's SideStream); COEB_SIDE_STREAM=0 disables
    SideStream side{};
    bool side_init = false;
    bool side_shared = false;                 // side.s is the device's shared side stream
    hipEvent_t ev_tprep = nullptr, ev_pose = nullptr;
    bool pose_pending = false;
    // batch tracking state: Observations() the matcher gave the LastFrame points, the frames and
    // min_matches of the last coeb_pose_batch_device (TrackLocalMap continues that batch)
    int batch_nobs = 2, pose_frames = 0, pose_min_matches = 20;
    hipEvent_t ev_tlm = nullptr;
    int tlm_frames = 0;
    // geometry of the last moving-object batch whose results the flow scratch still holds
    // (pairs == 0: none), for flow_counts / flow_pair
    struct { int w, h, pairs; } pmo_last{0, 0, 0};
    // pinned host staging of the host-buffer entry points: their inputs are packed here and
    // moved in one copy (a dozen small pageable copies cost more than the kernels)
    uint8_t* pin = nullptr;
    uint8_t* pin_dev = nullptr;        // the same page-locked bytes as the device addresses them
    size_t pin_n = 0;
};

// records msg as the context's (c may be null) and the calling thread's last error; returns code
int set_err(coeb_ctx* c, int code, const std::string& msg);
int hip_err(coeb_ctx* c, hipError_t e, const char* where);
#define HIP_TRY(ctx, expr)                                          \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return hip_err((ctx), _e, #expr);     \
    } while (0)

// The context stream, after it has been made to wait for every chunk stream of the last
// batch (so work enqueued on it sees the batch's results).
hipStream_t main_stream(coeb_ctx* c);
void join_pose(coeb_ctx* c);                    // the context stream waits for the last batch pose
int quiesce(coeb_ctx* c);                       // nothing enqueued by the context is running afterwards
const SideStream* side_stream(coeb_ctx* c);     // launch_extract's side stream, or null when disabled
void kfdb_release_all(coeb_ctx* c);             // coeb_kfdb.hip: coeb_destroy frees the databases' device memory
// coeb_capi.hip: the camera, the context's scale factors and mfLogScaleFactor as the matchers read them
MatchCam make_cam(const coeb_ctx* c, const coeb_camera* cam);

// a holds at least max(count * sizeof(T), 256) bytes afterwards; it only grows
template <class T>
int ensure(coeb_ctx* c, DevArr<T>& a, size_t count)
{
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    if (a.bytes >= bytes) return 0;
    if (a.p) {
        int rc = quiesce(c);          // work in flight on any of the context's streams may read it
        if (rc) return rc;
        (void)hipFree(a.p);
    }
    a.p = nullptr;
    a.bytes = 0;
    hipError_t e = hipMalloc(&a.p, bytes);
    if (e != hipSuccess) {
        a.p = nullptr;
        return set_err(c, COEB_ENOMEM, std::string("hipMalloc ") + a.name + ": " + hipGetErrorString(e));
    }
    a.bytes = bytes;
    return 0;
}

// Inputs of one call packed at 16-byte aligned offsets of the pinned staging buffer, moved to
// the device in one copy; fill() parts are constant bytes (absent optional arrays).
struct Pack {
    struct Part { const void* p; size_t n; int fill; };
    std::vector<Part> parts;
    size_t total = 0;
    size_t add(const void* p, size_t n) { return put(Part{p, n, -1}); }
    size_t fill(int byte, size_t n) { return put(Part{nullptr, n, byte}); }
    size_t put(Part q)
    {
        const size_t off = total;
        parts.push_back(q);
        total = (total + q.n + 15) & ~(size_t)15;
        return off;
    }
};

int pinned(coeb_ctx* c, size_t bytes);          // the page-locked buffer holds at least bytes afterwards
// pack -> pinned -> one H2D copy into the "stage" device buffer; *dbase = its device address
int stage_in(coeb_ctx* c, const Pack& pk, uint8_t** dbase, hipStream_t s);

// The staged region of one host-array call, at the same offsets of the "stage" device
// buffer and of the page-locked buffer: the packed inputs (uploaded in one copy; results that have
// an initial value are uploaded with them), then what take() hands out behind them at 16-byte
// rounded offsets -- first the results the kernels write, which finish() copies back in one piece
// together with the uploaded results in front of them, then scratch -- and, for a call that reads
// the device error word, the word's 16-byte slot of the page-locked buffer at the region's end.
struct Staged {
    Pack pk;
    size_t at = 0;                  // the region's end once take() has been called
    uint8_t* dbase = nullptr;       // stage(): the region on the device
    uint8_t* pin = nullptr;         //          and its page-locked copy
    size_t add(const void* p, size_t n) { return pk.add(p, n); }
    size_t fill(int byte, size_t n) { return pk.fill(byte, n); }
    size_t end() const { return std::max(at, pk.total); }
    size_t take(size_t bytes)
    {
        const size_t o = end();
        at = (o + bytes + 15) & ~(size_t)15;
        return o;
    }
    template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(dbase + off); }
    template <class T> const T* host(size_t off) const { return reinterpret_cast<const T*>(pin + off); }
    // both buffers sized for the region (with_err: and the error-word slot), the inputs enqueued on s
    int stage(coeb_ctx* c, hipStream_t s, bool with_err);
    // behind the kernels: one D2H copy of [from, to), the error word when asked, the call's one
    // synchronisation, and the verdict on the word
    int finish(coeb_ctx* c, hipStream_t s, size_t from, size_t to, bool with_err);
};

// coeb_bow.hip, called by coeb_capi.hip (coeb_track_reference_keyframe): Frame::ComputeBoW's transform and
// SearchByBoW on device arrays.  launch_transform: descriptor i of frame f at d_desc + (f * stride + i) * 32,
// d_counts ? d_counts[f] : n_fixed of them; d_word / d_node [F][stride].
double word_weight(const coeb_ctx* c, int word);            // of a word id the transform returned (-1: 0.0)
int launch_transform(coeb_ctx* c, const uint8_t* d_desc, const int* d_counts, int n_fixed, int stride, int F,
                     int levelsup, int* d_word, int* d_node, hipStream_t s);
struct BowSearch {
    const uint8_t* kf_valid; const uint8_t* kf_desc; const int* kf_node; const float* kf_angle; int kf_n;
    const uint8_t* cur_desc; const int* cur_node; const float* cur_angle; int cur_n;
    int* match;     // [max(cur_n, 1) + 1]: the KeyFrame index per frame feature (-1: none), then nmatches
};
int bow_search_bufs(coeb_ctx* c, int kf_n, int cur_n);      // the search's scratch, before anything is enqueued
int launch_search_by_bow(coeb_ctx* c, const BowSearch& a, float nnratio, int check_ori, hipStream_t s);

// coeb_flow.hip / coeb_frame.hip, called by coeb_capi.hip
int pmo_batch(coeb_ctx* c, const uint8_t* d_gray, int F, int w, int h, float* tm_out, int* ntm_out, int tm_cap);
int flow_counts(coeb_ctx* c, int* out, int cap, int* npairs);
// one pair's block of the flow scratch as coeb_debug_read("flow_pair") returns it
constexpr int kFlowPairPts = 1024;
struct FlowPairRecord {
    int32_t npts;                       // corners of the pair's previous frame (-1: sort capacity exceeded)
    int32_t nf;                         // |F_prepoint|: pairs that entered findFundamentalMat
    double F[9];
    float pts[2 * kFlowPairPts];        // sub-pixel corners
    float nxt[2 * kFlowPairPts];        // LK next points
    uint8_t status[kFlowPairPts];       // LK status
    uint8_t state[kFlowPairPts];        // after the SAD and edge test
};
int flow_pair(coeb_ctx* c, int z, FlowPairRecord* out);
int blur_flags_batch(coeb_ctx* c, const uint8_t* d_gray, int W, int H, const float* d_boxes, const int* d_box_off, int F,
                     int* d_box_frame, int nbox, int* d_out, hipStream_t s);

// coeb_flow.hip / coeb_frame.hip, called by coeb_rgbd_stream_frame (coeb_capi.hip): Frame::ProcessMovingObject
// in the pieces a frame stream launches, on memory the stream owns (never the context's flow scratch).
// What the chain keeps of one w x h frame (a slot of the stream, coeb_rgbd_stream_host.hpp):
struct StreamFlowFrame {
    uint8_t* gray;                      // level 0, pitch w
    uint8_t* lvl[8];                    // LK levels 1.. (pitch = level width)
    void* der[8];                       // Scharr planes of levels 0..
    float* pts; int* npts;              // refined corners, their count (-1: more candidates than the selection covers)
};
size_t stream_flow_corner_scratch(int w, int h);     // bytes stream_flow_corners needs
size_t stream_flow_track_scratch();                  // bytes stream_flow_track needs
int stream_flow_levels(int w, int h);                // LK pyramid levels the kernels build for a w x h frame
int stream_flow_init(coeb_ctx* c, uint8_t* corner_scratch);                         // cornerSubPix's weights (synchronous)
int stream_flow_pyramid(coeb_ctx* c, const StreamFlowFrame& f, int w, int h, hipStream_t s);      // k_pyr_down per level
// goodFeaturesToTrack, cornerSubPix and the Scharr derivatives of f: all the chain does on imGrayPre alone
int stream_flow_corners(coeb_ctx* c, const StreamFlowFrame& f, int w, int h, uint8_t* scratch, hipStream_t s);
// k_lk from prev's corners into cur, then k_fm: T_M into tm (tm_cap points), |T_M| or -1 into *ntm
int stream_flow_track(coeb_ctx* c, const StreamFlowFrame& prev, const StreamFlowFrame& cur, int w, int h, uint8_t* scratch,
                      float* tm, int* ntm, int tm_cap, hipStream_t s);
// GrabImageRGBD's cvtColor of one staged frame (k_rgbd), and the blur flags of its boxes (k_blur_flags)
int launch_rgbd_gray(coeb_ctx* c, const uint8_t* d_img, int row_bytes, int channels, int rgb_order, int W, int H,
                     uint8_t* d_gray, hipStream_t s);
int launch_blur_flags(coeb_ctx* c, const uint8_t* d_gray, int W, int H, const float* d_boxes, int nbox, int* d_out,
                      hipStream_t s);
