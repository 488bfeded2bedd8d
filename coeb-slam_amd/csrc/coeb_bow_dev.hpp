// coeb_bow_dev.hpp -- what the two SearchByBoW paths share (coeb_bow.hip: one keyframe per call,
// coeb_kfdb.hip: the keyframe database's candidates in one launch): the feature-vector CSR's
// layout and its launcher, the per-node matching walk and the rotation filter
// (src/ORBmatcher.cc:159-288) as device functions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coeb_ctx.hpp"
#include "coeb_match_dev.hpp"

constexpr int kBowThreads = 256;
constexpr int kBowMax = kCurMax;        // features per frame the CSR and the matcher take
constexpr int TH_LOW = 50;
constexpr int kBowWaves = kBowThreads / 64;
constexpr int kTile = 128;
constexpr int kCsrThreads = 1024;

// The FeatureVector of one frame as a CSR (k_bow_csr, coeb_bow.hip):
//   out[0] = nd distinct nodes, out[1] = m listed features,
//   out + 4: node[cap] ascending, then off[cap + 1], then idx[cap]   (cap = max(n, 1))
struct CsrSide { const int* node; const uint8_t* valid; int n; int* out; };
struct CsrArgs { CsrSide side[2]; int* clear_m1; int clear_n; int* clear_0; int clear_0n; };
inline int csr_ints(int n) { return 4 + 3 * std::max(n, 1) + 1; }
// k_bow_csr over a.side[0 .. sides); the last workgroup also clears a.clear_* (coeb_bow.hip)
void launch_bow_csr(coeb_ctx* c, const CsrArgs& a, int sides, hipStream_t s);

struct BowSide { const uint8_t* desc; const float* angle; const int* csr; int n; };

// One wave per node w of the KeyFrame's FeatureVector; a node the frame does not have ends at once.
// A frame feature lies under one node only, so the nodes are independent; within a node the
// KeyFrame features are taken in order, each against the node's frame features not yet given
// away (:205-226).  Lane l looks at list positions l, l + 64, ..: its "taken" bits are a private
// 64-bit mask (a list holds at most kBowMax < 4096 features), the frame descriptors of a list of
// up to kTile sit in LDS (s_desc, this wave's [8][kTile], word-major, so a wave reads consecutive
// banks), longer lists are read from global memory.  best1 = min of (dist << 16 | position): the
// first strict minimum; best2 = the second order statistic, merged as min(b2, b2', max(b1, b1')).
// kValid: the KeyFrame's CSR lists every feature with a node and valid[ikf] is tested here, as the
// reference's loop does (:199-203); otherwise the CSR holds the valid features only.
template <bool kValid>
__device__ __forceinline__ void bow_match_node(const BowSide& kf, const BowSide& cur, const uint8_t* __restrict__ valid,
                                               int w, float nnratio, int check_ori, int* match, int* bin, int* hist,
                                               uint32_t (*s_desc)[kTile], int lane)
{
    const int kcap = max(kf.n, 1), ccap = max(cur.n, 1);
    const int* k_node = kf.csr + 4;
    const int* k_off = k_node + kcap;
    const int* k_idx = k_off + kcap + 1;
    const int* c_node = cur.csr + 4;
    const int* c_off = c_node + ccap;
    const int* c_idx = c_off + ccap + 1;
    if (w >= kf.csr[0]) return;                    // wave-uniform from here on
    const int node = k_node[w];
    int lo = 0, hi = cur.csr[0];
    while (lo < hi) {                              // lower bound of node among the frame's nodes
        const int mid = (lo + hi) >> 1;
        if (c_node[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= cur.csr[0] || c_node[lo] != node) return;
    const int c0 = c_off[lo], len = c_off[lo + 1] - c0;
    const int k0 = k_off[w], k1 = k_off[w + 1];
    const int iters = (len + 63) >> 6;
    const bool tile = len <= kTile;
    if (tile) {
        for (int p = lane; p < len; p += 64) {
            const uint4* d = reinterpret_cast<const uint4*>(cur.desc + (int64_t)c_idx[c0 + p] * 32);
            const uint4 d0 = d[0], d1 = d[1];
            s_desc[0][p] = d0.x; s_desc[1][p] = d0.y; s_desc[2][p] = d0.z; s_desc[3][p] = d0.w;
            s_desc[4][p] = d1.x; s_desc[5][p] = d1.y; s_desc[6][p] = d1.z; s_desc[7][p] = d1.w;
        }
    }
    // no barrier: position p is written and read by lane p % 64 only
    uint64_t taken = 0;
    for (int kq = k0; kq < k1; kq++) {
        const int ikf = __builtin_amdgcn_readfirstlane(k_idx[kq]);
        if (kValid && !valid[ikf]) continue;       // wave-uniform
        uint32_t q[8];
        {
            const uint4* d = reinterpret_cast<const uint4*>(kf.desc + (int64_t)ikf * 32);
            const uint4 d0 = d[0], d1 = d[1];
            q[0] = d0.x; q[1] = d0.y; q[2] = d0.z; q[3] = d0.w;
            q[4] = d1.x; q[5] = d1.y; q[6] = d1.z; q[7] = d1.w;
        }
        uint32_t b1 = (256u << 16) | 0xFFFFu, b2 = 256;
        for (int it = 0; it < iters; it++) {
            const int p = it * 64 + lane;
            if (p >= len || ((taken >> it) & 1)) continue;
            uint32_t c[8];
            if (tile) {
#pragma unroll
                for (int k = 0; k < 8; k++) c[k] = s_desc[k][p];
            } else {
                const uint4* d = reinterpret_cast<const uint4*>(cur.desc + (int64_t)c_idx[c0 + p] * 32);
                const uint4 d0 = d[0], d1 = d[1];
                c[0] = d0.x; c[1] = d0.y; c[2] = d0.z; c[3] = d0.w;
                c[4] = d1.x; c[5] = d1.y; c[6] = d1.z; c[7] = d1.w;
            }
            const uint32_t dist = (uint32_t)hamming32(q, c);
            if (dist < (b1 >> 16)) { b2 = b1 >> 16; b1 = (dist << 16) | (uint32_t)p; }   // p ascends per lane
            else if (dist < b2) b2 = dist;
        }
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) {
            const uint32_t o1 = (uint32_t)__shfl_xor((int)b1, x), o2 = (uint32_t)__shfl_xor((int)b2, x);
            b2 = min(min(b2, o2), max(b1, o1) >> 16);
            b1 = min(b1, o1);
        }
        const int d1 = (int)(b1 >> 16), p1 = (int)(b1 & 0xFFFFu);
        if (d1 <= TH_LOW && (float)d1 < nnratio * (float)(int)b2) {
            if ((p1 & 63) == lane) taken |= (uint64_t)1 << (p1 >> 6);
            if (lane == 0) {
                const int icur = c_idx[c0 + p1];
                match[icur] = ikf;
                if (check_ori) {
                    int b = rot_bin(kf.angle[ikf], cur.angle[icur]);
                    if (b < 0 || b >= HISTO_LENGTH) b = HISTO_LENGTH;            // the reference asserts; dropped below
                    else atomicAdd(&hist[b], 1);
                    bin[icur] = b;
                }
            }
        }
    }
}

// The rotation-consistency filter over one frame's matches (:267-285) and their count, by one
// workgroup of kCsrThreads: inout[i] for i < n, *nm_out = nmatches.  s_ind[3] and *s_cnt are LDS.
__device__ __forceinline__ void bow_rot_filter(int* inout, const int* bin, const int* hist, int n, int check_ori,
                                               int* nm_out, int* s_ind, int* s_cnt)
{
    const int tid = threadIdx.x;
    if (tid == 0) {
        int i1 = -1, i2 = -1, i3 = -1;
        if (check_ori) three_maxima(hist, i1, i2, i3);
        s_ind[0] = i1; s_ind[1] = i2; s_ind[2] = i3;
        *s_cnt = 0;
    }
    __syncthreads();
    int kept = 0;
    for (int i = tid; i < n; i += kCsrThreads) {
        int m = inout[i];
        if (m >= 0 && check_ori) {
            const int b = bin[i];
            if (b != s_ind[0] && b != s_ind[1] && b != s_ind[2]) { m = -1; inout[i] = -1; }
        }
        kept += m >= 0;
    }
    if (kept) atomicAdd(s_cnt, kept);
    __syncthreads();
    if (tid == 0) *nm_out = *s_cnt;
}
