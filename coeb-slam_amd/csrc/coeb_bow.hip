// coeb_bow.hip -- the bag-of-words front end of TrackReferenceKeyFrame / Relocalization:
//   Frame::ComputeBoW -> TemplatedVocabulary::transform(feature, word, weight, &nid, levelsup)
//                                                  src/Frame.cc:570-577             (k_bow_transform)
//   DBoW2::FeatureVector (node id -> feature indices) as a CSR                       (k_bow_csr)
//   ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
//                                                  src/ORBmatcher.cc:159-288        (k_match_bow, k_bow_rot)
// DBoW2 is not a dependency: the vocabulary is plain data (coeb_voc.cpp) and the algorithms are
// the ones DESIGN.md s4.12 spells out; parity against DBoW2 itself is UNPINNED.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "coeb_bow_dev.hpp"

namespace {

// Minimum of v over the 16 lanes of a DPP row, in every lane: xor 1, xor 2 (quad permutes), then
// the half-row and row mirrors (lane i <-> 7 - i, i <-> 15 - i), each of which pairs groups
// that already agree.
__device__ __forceinline__ uint32_t row_min16(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}

// ============================ k_bow_transform ============================
// G lanes per descriptor (16: a DPP row, four descriptors per wave; 32 for k > 16).  Per level
// lane j loads child j's descriptor and record (independent loads, issued together), the group
// takes the minimum of (distance << 8 | j) -- so the first child wins a tie, as the reference's
// strict < does -- and the winner's record comes from its lane by a shuffle: one memory round
// trip per level.  Lanes without a child carry distance 257.
// recs / vdesc: the vocabulary by slot (coeb_voc.hpp).  Descriptor i of frame f at
// desc + (f * stride + i) * 32, n = counts ? counts[f] : n_fixed; outputs [f][stride], -1 past n.
// node = the id of the ancestor at level nid_level (0: the root when nid_level <= 0; the leaf
// when it lies above that level), or -1 when the word's weight is not > 0.
template <int G>
__global__ __launch_bounds__(kBowThreads) void k_bow_transform(const VocRec* __restrict__ recs,
                                                               const uint8_t* __restrict__ vdesc,
                                                               const uint8_t* __restrict__ desc,
                                                               const int* __restrict__ counts, int n_fixed, int stride,
                                                               int nid_level, int* __restrict__ word,
                                                               int* __restrict__ node)
{
    const int f = blockIdx.y;
    const int n = counts ? min(counts[f], stride) : n_fixed;
    const int gl = threadIdx.x % G;
    const int i = blockIdx.x * (kBowThreads / G) + threadIdx.x / G;
    if (i >= stride) return;
    const int64_t o = (int64_t)f * stride + i;
    if (i >= n) {                              // G-uniform
        if (gl == 0) { word[o] = -1; node[o] = -1; }
        return;
    }
    uint32_t q[8];
    {
        const uint4* d = reinterpret_cast<const uint4*>(desc + o * 32);
        const uint4 d0 = d[0], d1 = d[1];
        q[0] = d0.x; q[1] = d0.y; q[2] = d0.z; q[3] = d0.w;
        q[4] = d1.x; q[5] = d1.y; q[6] = d1.z; q[7] = d1.w;
    }
    VocRec cur = recs[0];
    int level = 0, nid = 0;
    do {
        level++;
        const int first = cur.child_first, cnt = cur.child_count;
        uint32_t key = (257u << 8) | (uint32_t)gl;
        int4 r = make_int4(0, 0, -1, 0);
        if (gl < cnt) {
            const uint4* d = reinterpret_cast<const uint4*>(vdesc + (int64_t)(first + gl) * 32);
            const uint4 d0 = d[0], d1 = d[1];
            r = *reinterpret_cast<const int4*>(recs + first + gl);
            const uint32_t c[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            key = ((uint32_t)hamming32(q, c) << 8) | (uint32_t)gl;
        }
        key = row_min16(key);
        if (G == 32) key = min(key, (uint32_t)__shfl_xor((int)key, 16));
        const int win = (int)(key & 0xFFu);
        cur.child_first = __shfl(r.x, win, G);
        cur.child_count = __shfl(r.y, win, G);
        cur.word = __shfl(r.z, win, G);
        cur.id_flag = (uint32_t)__shfl(r.w, win, G);
        if (level == nid_level) nid = (int)(cur.id_flag & ~kVocPositive);
    } while (cur.child_count != 0);
    if (level < nid_level) nid = (int)(cur.id_flag & ~kVocPositive);      // a leaf above nid_level
    if (gl == 0) {
        word[o] = cur.word;
        node[o] = (cur.id_flag & kVocPositive) ? nid : -1;
    }
}

// ============================== k_bow_csr ==============================
// The FeatureVector of one frame as a CSR, one workgroup per side: features with node id >= 0
// (and valid[i], when given) sorted by (node id, index) with a counting (rank) sort -- the rank
// of a feature is the number of features before it in that order, counted against the node ids
// in LDS -- then the distinct node ids by a scan over the run heads.
// The layout of `out`, CsrSide and CsrArgs: coeb_bow_dev.hpp.
constexpr int kCsrSlots = 4096;         // >= kBowMax + 1

__global__ __launch_bounds__(kCsrThreads) void k_bow_csr(CsrArgs a)
{
    __shared__ int s_key[kCsrSlots], s_node[kCsrSlots], s_idx[kCsrSlots];
    __shared__ int s_scan[kCsrThreads];
    __shared__ int s_m;
    const int tid = threadIdx.x;
    const CsrSide sd = a.side[blockIdx.x];
    if (blockIdx.x == gridDim.x - 1) {             // the matcher's outputs, cleared beside the sort
        for (int i = tid; i < a.clear_n; i += kCsrThreads) a.clear_m1[i] = -1;
        for (int i = tid; i < a.clear_0n; i += kCsrThreads) a.clear_0[i] = 0;
    }
    const int n = min(sd.n, kBowMax), cap = max(n, 1);
    int* o_node = sd.out + 4;
    int* o_off = o_node + cap;
    int* o_idx = o_off + cap + 1;
    if (tid == 0) s_m = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += kCsrThreads) {
        int k = sd.node[i];
        if (k < 0 || (sd.valid && !sd.valid[i])) k = 0x7fffffff;
        else mine++;
        s_key[i] = k;
    }
    if (mine) atomicAdd(&s_m, mine);
    __syncthreads();
    const int m = s_m;
    for (int i = tid; i < n; i += kCsrThreads) {
        const int k = s_key[i];
        if (k == 0x7fffffff) continue;
        int rank = 0;
        for (int j = 0; j < i; j++) rank += s_key[j] <= k;
        for (int j = i + 1; j < n; j++) rank += s_key[j] < k;
        s_node[rank] = k;
        s_idx[rank] = i;
    }
    __syncthreads();
    // run heads, kCsrSlots / kCsrThreads consecutive positions per thread, then their scan
    constexpr int C = kCsrSlots / kCsrThreads;
    int heads = 0;
    for (int p = tid * C; p < min(tid * C + C, m); p++) heads += p == 0 || s_node[p] != s_node[p - 1];
    s_scan[tid] = heads;
    __syncthreads();
    for (int d = 1; d < kCsrThreads; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int dpos = s_scan[tid] - heads;
    for (int p = tid * C; p < min(tid * C + C, m); p++) {
        if (p == 0 || s_node[p] != s_node[p - 1]) {
            o_node[dpos] = s_node[p];
            o_off[dpos] = p;
            dpos++;
        }
        o_idx[p] = s_idx[p];
    }
    if (tid == kCsrThreads - 1) {
        const int nd = s_scan[tid];
        sd.out[0] = nd;
        sd.out[1] = m;
        o_off[nd] = m;
    }
}

// ============================= k_match_bow =============================
// One wave per node of the KeyFrame's FeatureVector (bow_match_node, coeb_bow_dev.hpp); the
// KeyFrame's CSR holds its valid features only.
struct BowMatch { BowSide kf, cur; float nnratio; int check_ori; int* match; int* bin; int* hist; };

__global__ __launch_bounds__(kBowThreads) void k_match_bow(BowMatch a)
{
    __shared__ uint32_t s_desc[kBowWaves][8][kTile];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bow_match_node<false>(a.kf, a.cur, nullptr, blockIdx.x * kBowWaves + wv, a.nnratio, a.check_ori, a.match, a.bin,
                          a.hist, s_desc[wv], lane);
}

// The rotation-consistency filter over the whole frame (:267-285) and the match count:
// inout[i] for i < n, inout[cap] = nmatches.
__global__ __launch_bounds__(kCsrThreads) void k_bow_rot(int* inout, const int* bin, const int* hist, int n, int cap,
                                                         int check_ori)
{
    __shared__ int s_ind[3], s_cnt;
    bow_rot_filter(inout, bin, hist, n, check_ori, inout + cap, s_ind, &s_cnt);
}

}  // namespace

double word_weight(const coeb_ctx* c, int word)
{
    return (word >= 0 && word < (int)c->voc.word_weight.size()) ? c->voc.word_weight[word] : 0.0;
}

int launch_transform(coeb_ctx* c, const uint8_t* d_desc, const int* d_counts, int n_fixed, int stride, int F,
                     int levelsup, int* d_word, int* d_node, hipStream_t s)
{
    const int nid_level = c->voc.L - levelsup;
    const int G = c->voc.k <= 16 ? 16 : 32;
    const dim3 grid((stride + kBowThreads / G - 1) / (kBowThreads / G), F);
    prof_begin(&c->hook, "k_bow_transform", s);
    if (G == 16)
        hipLaunchKernelGGL(k_bow_transform<16>, grid, dim3(kBowThreads), 0, s, c->bow.v_rec.p, c->bow.v_desc.p, d_desc,
                           d_counts, n_fixed, stride, nid_level, d_word, d_node);
    else
        hipLaunchKernelGGL(k_bow_transform<32>, grid, dim3(kBowThreads), 0, s, c->bow.v_rec.p, c->bow.v_desc.p, d_desc,
                           d_counts, n_fixed, stride, nid_level, d_word, d_node);
    prof_end(&c->hook, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void launch_bow_csr(coeb_ctx* c, const CsrArgs& a, int sides, hipStream_t s)
{
    prof_begin(&c->hook, "k_bow_csr", s);
    hipLaunchKernelGGL(k_bow_csr, dim3(sides), dim3(kCsrThreads), 0, s, a);
    prof_end(&c->hook, s);
}

// launch_search_by_bow's scratch: the two CSRs (m_csr) and bin[max(cur_n, 1)] + hist[32] (m_aux)
int bow_search_bufs(coeb_ctx* c, int kf_n, int cur_n)
{
    int rc;
    if ((rc = ensure(c, c->bow.m_csr, (size_t)csr_ints(kf_n) + csr_ints(cur_n)))) return rc;
    return ensure(c, c->bow.m_aux, (size_t)std::max(cur_n, 1) + 32);
}

// SearchByBoW on device arrays: k_bow_csr (both sides; it clears the outputs) -> k_match_bow -> k_bow_rot
int launch_search_by_bow(coeb_ctx* c, const BowSearch& a, float nnratio, int check_ori, hipStream_t s)
{
    const int nq = a.kf_n, n = a.cur_n, cs = std::max(n, 1);
    int* csr_k = c->bow.m_csr.p;
    int* csr_c = csr_k + csr_ints(nq);
    int* d_bin = c->bow.m_aux.p;
    int* d_hist = d_bin + cs;
    CsrArgs ca{};
    ca.side[0] = CsrSide{a.kf_node, a.kf_valid, nq, csr_k};
    ca.side[1] = CsrSide{a.cur_node, nullptr, n, csr_c};
    ca.clear_m1 = a.match; ca.clear_n = cs + 1;
    ca.clear_0 = d_bin; ca.clear_0n = cs + 32;
    launch_bow_csr(c, ca, 2, s);
    BowMatch bm;
    bm.kf = BowSide{a.kf_desc, a.kf_angle, csr_k, nq};
    bm.cur = BowSide{a.cur_desc, a.cur_angle, csr_c, n};
    bm.nnratio = nnratio; bm.check_ori = check_ori ? 1 : 0;
    bm.match = a.match; bm.bin = d_bin; bm.hist = d_hist;
    if (nq && n) {
        prof_begin(&c->hook, "k_match_bow", s);
        hipLaunchKernelGGL(k_match_bow, dim3((nq + kBowWaves - 1) / kBowWaves), dim3(kBowThreads), 0, s, bm);
        prof_end(&c->hook, s);
    }
    prof_begin(&c->hook, "k_bow_rot", s);
    hipLaunchKernelGGL(k_bow_rot, dim3(1), dim3(kCsrThreads), 0, s, a.match, d_bin, d_hist, n, cs, bm.check_ori);
    prof_end(&c->hook, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" {

int coeb_bow_set_vocabulary(coeb_ctx* c, const coeb_voc* voc)
{
    if (!c || !voc || voc->nnodes < 2) return set_err(c, COEB_EINVAL, "coeb_bow_set_vocabulary: invalid arguments");
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = quiesce(c))) return rc;              // a transform in flight reads the previous tables
    c->voc.k = 0;
    if ((rc = ensure(c, c->bow.v_rec, (size_t)voc->nnodes)) || (rc = ensure(c, c->bow.v_desc, (size_t)voc->nnodes * 32)))
        return rc;
    HIP_TRY(c, hipMemcpy(c->bow.v_rec.p, voc->rec.data(), (size_t)voc->nnodes * sizeof(VocRec), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->bow.v_desc.p, voc->desc.data(), (size_t)voc->nnodes * 32, hipMemcpyHostToDevice));
    c->voc.word_weight = voc->word_weight;
    c->voc.k = voc->k; c->voc.L = voc->L; c->voc.nnodes = voc->nnodes;
    return COEB_OK;
}

int coeb_bow_transform(coeb_ctx* c, const uint8_t* desc, int n, int levelsup, int32_t* word_out, int32_t* node_out,
                       double* weight_out, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int fv_cap, int* nfv_out)
{
    if (!c || n < 0 || levelsup < 0 || (n && !desc)) return set_err(c, COEB_EINVAL, "coeb_bow_transform: invalid arguments");
    if (nfv_out) *nfv_out = 0;
    if (!c->voc.k) return set_err(c, COEB_EINVAL, "coeb_bow_transform: no vocabulary (coeb_bow_set_vocabulary)");
    if (n > kBowMax) return set_err(c, COEB_EINVAL, "coeb_bow_transform: more than 4095 descriptors");
    const bool want_fv = fv_node || fv_off || fv_idx;
    if (want_fv && (!fv_node || !fv_off || !fv_idx || !nfv_out || fv_cap < 0))
        return set_err(c, COEB_EINVAL, "coeb_bow_transform: incomplete feature-vector outputs");
    (void)hipSetDevice(c->device);
    const int cap = std::max(n, 1);
    hipStream_t s = main_stream(c);
    Staged st;
    const size_t o_d = st.add(desc, (size_t)n * 32);
    const size_t o_w = st.take((size_t)cap * 4), o_n = st.take((size_t)cap * 4), o_csr = st.take((size_t)csr_ints(n) * 4);
    int rc;
    if ((rc = st.stage(c, s, false))) return rc;
    if (n && launch_transform(c, st.dev<uint8_t>(o_d), nullptr, n, n, 1, levelsup, st.dev<int>(o_w), st.dev<int>(o_n), s))
        return hip_err(c, hipGetLastError(), "k_bow_transform");
    CsrArgs ca{};
    ca.side[0] = CsrSide{st.dev<int>(o_n), nullptr, n, st.dev<int>(o_csr)};
    launch_bow_csr(c, ca, 1, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_w, st.end(), false))) return rc;
    const int32_t* h_word = st.host<int32_t>(o_w);
    const int32_t* h_csr = st.host<int32_t>(o_csr);
    if (word_out) memcpy(word_out, h_word, (size_t)n * 4);
    if (node_out) memcpy(node_out, st.host<int32_t>(o_n), (size_t)n * 4);
    for (int i = 0; weight_out && i < n; i++) weight_out[i] = word_weight(c, h_word[i]);
    if (want_fv) {
        const int nd = h_csr[0], m = h_csr[1];
        *nfv_out = nd;
        if (nd > fv_cap) return set_err(c, COEB_ERANGE, "coeb_bow_transform: feature vector exceeds fv_cap nodes");
        memcpy(fv_node, h_csr + 4, (size_t)nd * 4);
        memcpy(fv_off, h_csr + 4 + cap, ((size_t)nd + 1) * 4);
        memcpy(fv_idx, h_csr + 4 + 2 * cap + 1, (size_t)m * 4);
    }
    return COEB_OK;
}

int coeb_bow_batch_device(coeb_ctx* c, int levelsup)
{
    if (!c || levelsup < 0) return set_err(c, COEB_EINVAL, "coeb_bow_batch_device: invalid arguments");
    if (!c->voc.k) return set_err(c, COEB_EINVAL, "coeb_bow_batch_device: no vocabulary (coeb_bow_set_vocabulary)");
    if (!c->has_plan || c->batch_frames <= 0 || !c->ex.desc.p || !c->ex.counts.p)
        return set_err(c, COEB_EINVAL, "coeb_bow_batch_device: must follow a batch extraction");
    (void)hipSetDevice(c->device);
    const int F = c->batch_frames, K = c->plan.kcap;
    int rc;
    if ((rc = ensure(c, c->bow.b_word, (size_t)F * K)) || (rc = ensure(c, c->bow.b_node, (size_t)F * K))) return rc;
    hipStream_t s = main_stream(c);                 // joins the extraction's chunk streams
    c->bow_frames = 0;
    if (launch_transform(c, c->ex.desc.p, c->ex.counts.p, 0, K, F, levelsup, c->bow.b_word.p, c->bow.b_node.p, s))
        return hip_err(c, hipGetLastError(), "k_bow_transform");
    c->bow_frames = F;
    return COEB_OK;
}

int coeb_batch_bow_results(coeb_ctx* c, const int32_t** d_word, const int32_t** d_node)
{
    if (!c || !c->bow_frames || c->bow_frames != c->batch_frames)
        return set_err(c, COEB_EINVAL, "coeb_batch_bow_results: no coeb_bow_batch_device on the last batch");
    if (d_word) *d_word = c->bow.b_word.p;
    if (d_node) *d_node = c->bow.b_node.p;
    return COEB_OK;
}

int coeb_match_bow(coeb_ctx* c, const coeb_bow_keyframe* kf, const coeb_bow_frame* cur, float nnratio,
                   int check_orientation, int32_t* match_out, int* nmatches)
{
    if (!c || !kf || !cur || !nmatches) return set_err(c, COEB_EINVAL, "coeb_match_bow: invalid arguments");
    *nmatches = 0;
    const int nq = kf->n, n = cur->n;
    if (nq < 0 || n < 0) return set_err(c, COEB_EINVAL, "negative frame / keyframe size");
    if (nq > kBowMax || n > kBowMax) return set_err(c, COEB_EINVAL, "coeb_match_bow: more than 4095 features");
    if (nq && (!kf->valid || !kf->descriptor || !kf->node_id || !kf->angle))
        return set_err(c, COEB_EINVAL, "coeb_match_bow: missing keyframe arrays");
    if (n && (!cur->descriptor || !cur->node_id || !cur->angle || !match_out))
        return set_err(c, COEB_EINVAL, "coeb_match_bow: missing current-frame arrays");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1);
    int rc;
    if ((rc = bow_search_bufs(c, nq, n))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    const size_t o_v = st.add(kf->valid, (size_t)nq), o_kd = st.add(kf->descriptor, (size_t)nq * 32);
    const size_t o_kn = st.add(kf->node_id, (size_t)nq * 4), o_ka = st.add(kf->angle, (size_t)nq * 4);
    const size_t o_cd = st.add(cur->descriptor, (size_t)n * 32), o_cn = st.add(cur->node_id, (size_t)n * 4);
    const size_t o_ca = st.add(cur->angle, (size_t)n * 4);
    const size_t o_m = st.take(((size_t)cs + 1) * 4);
    if ((rc = st.stage(c, s, false))) return rc;
    BowSearch bs;
    bs.kf_valid = st.dev<uint8_t>(o_v); bs.kf_desc = st.dev<uint8_t>(o_kd); bs.kf_node = st.dev<int>(o_kn);
    bs.kf_angle = st.dev<float>(o_ka); bs.kf_n = nq;
    bs.cur_desc = st.dev<uint8_t>(o_cd); bs.cur_node = st.dev<int>(o_cn); bs.cur_angle = st.dev<float>(o_ca);
    bs.cur_n = n; bs.match = st.dev<int>(o_m);
    if (launch_search_by_bow(c, bs, nnratio, check_orientation, s)) return hip_err(c, hipGetLastError(), "launch_search_by_bow");
    if ((rc = st.finish(c, s, o_m, st.end(), false))) return rc;
    const int32_t* hout = st.host<int32_t>(o_m);
    if (n) memcpy(match_out, hout, (size_t)n * 4);
    *nmatches = hout[cs];
    return COEB_OK;
}

}  // extern "C"
