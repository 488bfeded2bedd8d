// The host half of the keyframe database (C++, no device code): BowVector filling as DBoW2's
// containers do it, and the list order / word threshold of DetectRelocalizationCandidates.
// Written from the definitions DESIGN.md s4.13 restates, not from DBoW2 (absent here; parity
// against it is UNPINNED).
#include <algorithm>
#include <cmath>
#include <map>
#include <numeric>
#include <vector>

#include "../../include/coeb_front.h"
#include "coeb_kfdb_host.hpp"

int kfdb_min_common(int max_common)
{
    const float m = (float)max_common * 0.8f;
    return (int)m;
}

int kfdb_sharing_order(const int32_t* common, const int32_t* first_word, const int64_t* seq, int nslots, int32_t* order)
{
    int m = 0;
    for (int s = 0; s < nslots; s++)
        if (common[s] > 0) order[m++] = s;
    std::sort(order, order + m, [&](int32_t a, int32_t b) {
        if (first_word[a] != first_word[b]) return first_word[a] < first_word[b];
        return seq[a] < seq[b];
    });
    return m;
}

bool kfdb_words_ascending(const int32_t* word, int nw)
{
    for (int i = 0; i < nw; i++)
        if (word[i] < 0 || (i && word[i] <= word[i - 1])) return false;
    return true;
}

extern "C" int coeb_bow_vector(const int32_t* word, const double* weight, const int32_t* node, int n, int normalize_l1,
                               int32_t* word_out, double* value_out, int cap, int* nw_out)
{
    if (n < 0 || cap < 0 || !nw_out || (n && (!word || !weight || !node)) || (cap && (!word_out || !value_out)))
        return COEB_EINVAL;
    *nw_out = 0;
    std::map<int32_t, double> bv;
    for (int i = 0; i < n; i++) {
        if (node[i] < 0) continue;
        // BowVector::addWeight: += when present, else insert
        std::map<int32_t, double>::iterator it = bv.lower_bound(word[i]);
        if (it != bv.end() && it->first == word[i]) it->second += weight[i];
        else bv.insert(it, std::make_pair(word[i], weight[i]));
    }
    if (normalize_l1) {
        double norm = 0.0;
        for (const auto& e : bv) norm += std::fabs(e.second);
        if (norm > 0.0)
            for (auto& e : bv) e.second /= norm;
    }
    *nw_out = (int)bv.size();
    if ((int)bv.size() > cap) return COEB_ERANGE;
    int k = 0;
    for (const auto& e : bv) {
        word_out[k] = e.first;
        value_out[k] = e.second;
        k++;
    }
    return COEB_OK;
}

// ---- SearchForTriangulation over stored keyframes: packing and argument rules ----
bool kfdb_pack_geometry(const coeb_keypoint* keys_un, const float* u_right, int n, int nlevels, KfdbGeo* out)
{
    for (int i = 0; i < n; i++) {
        const int oct = keys_un[i].octave;
        if (oct < 0 || oct >= nlevels) return false;
        out[i] = KfdbGeo{keys_un[i].x, keys_un[i].y, u_right[i], oct};
    }
    return true;
}

const char* kfdb_tri_check(const uint8_t* used, const uint8_t* geo, const int* n, int nslots, int slot1,
                           const uint8_t* has_mp1, const int32_t* slots2, int nnb, const uint8_t* const* has_mp2,
                           const float* F12, const float* epipole, const int32_t* match_out, const int32_t* nmatches)
{
    if (nnb < 0 || nnb > COEB_TRI_MAX_NEIGHBOURS) return "the neighbour count lies outside 0..32";
    if (slot1 < 0 || slot1 >= nslots || !used[slot1]) return "no keyframe in slot1";
    if (!geo[slot1]) return "slot1 has no geometry (coeb_kfdb_set_geometry)";
    if (nnb == 0) return nullptr;
    if (!slots2 || !has_mp2 || !F12 || !epipole || !nmatches) return "missing arrays";
    if (n[slot1] && (!has_mp1 || !match_out)) return "missing has_mp1 or match_out";
    for (int j = 0; j < nnb; j++) {
        const int s = slots2[j];
        if (s < 0 || s >= nslots || !used[s]) return "no keyframe in a neighbour's slot";
        if (!geo[s]) return "a neighbour's slot has no geometry (coeb_kfdb_set_geometry)";
        if (n[s] && !has_mp2[j]) return "missing has_mp2 mask";
    }
    return nullptr;
}

void kfdb_tri_pack(const int* n, const int32_t* slots2, int nnb, const uint8_t* const* has_mp2,
                   std::vector<uint8_t>& masks, std::vector<int32_t>& tab)
{
    tab.assign((size_t)nnb * 2, 0);
    size_t total = 0;
    for (int j = 0; j < nnb; j++) {
        tab[2 * j] = slots2[j];
        tab[2 * j + 1] = (int32_t)total;
        total += ((size_t)n[slots2[j]] + 15) & ~(size_t)15;
    }
    masks.assign(total, 0);
    for (int j = 0; j < nnb; j++) {
        const int nj = n[slots2[j]];
        if (nj) std::copy(has_mp2[j], has_mp2[j] + nj, masks.begin() + tab[2 * j + 1]);
    }
}

// ---- Fuse's search over stored keyframes: packing and argument rules ----
bool kfdb_grid_current(const KfdbGridRec& r, const coeb_camera* cam)
{
    return r.built && r.min_x == cam->min_x && r.max_x == cam->max_x && r.min_y == cam->min_y && r.max_y == cam->max_y;
}

const char* kfdb_fuse_check(const uint8_t* used, const uint8_t* geo, int nslots, const coeb_camera* cam,
                            const coeb_fuse_points* pts, const coeb_fuse_job* jobs, int njobs, float th,
                            const int32_t* best_idx, const int32_t* best_dist, int* code, int64_t* total)
{
    *code = COEB_EINVAL;
    *total = 0;
    if (!cam || !pts) return "missing camera or point list";
    if (njobs < 0 || njobs > COEB_FUSE_MAX_JOBS) return "the job count lies outside 0..128";
    if (!(th >= 0.0f) || !std::isfinite(th)) return "th is negative or not finite";
    if (!std::isfinite(cam->min_x) || !std::isfinite(cam->max_x) || !std::isfinite(cam->min_y) ||
        !std::isfinite(cam->max_y) || !(cam->max_x > cam->min_x) || !(cam->max_y > cam->min_y))
        return "camera bounds are not finite with max > min";
    const int n = pts->n;
    if (n < 0) return "negative point count";
    if (njobs && !jobs) return "missing job array";
    if (n && (!pts->valid || !pts->world_pos || !pts->normal || !pts->max_distance || !pts->min_distance || !pts->descriptor))
        return "missing point arrays";
    int64_t sum = 0;
    for (int j = 0; j < njobs; j++) {
        const coeb_fuse_job& b = jobs[j];
        if (b.slot < 0 || b.slot >= nslots || !used[b.slot]) return "no keyframe in a job's slot";
        if (!geo[b.slot]) return "a job's slot has no geometry (coeb_kfdb_set_geometry)";
        if (b.first < 0 || b.count < 0 || (int64_t)b.first + b.count > n) return "a job's range lies outside the list";
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(b.Rcw[k])) return "a job's pose is not finite";
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(b.tcw[k]) || !std::isfinite(b.Ow[k])) return "a job's pose is not finite";
        sum += b.count;
    }
    if (sum && (!best_idx || !best_dist)) return "missing output arrays";
    // PredictScale's (int)ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) is undefined otherwise
    for (int q = 0; q < n; q++) {
        if (!pts->valid[q]) continue;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(pts->world_pos[3 * q + k]) || !std::isfinite(pts->normal[3 * q + k]))
                return "non-finite position or normal of a valid point";
        const float mn = pts->min_distance[q], mx = pts->max_distance[q];
        if (!(mn > 0.0f && mn <= mx && std::isfinite(mx))) return "distance range of a valid point is not 0 < min <= max < inf";
    }
    *code = COEB_ERANGE;
    if (sum > COEB_FUSE_MAX_PAIRS) return "more than COEB_FUSE_MAX_PAIRS (job, point) pairs";
    if (n > COEB_FUSE_MAX_PAIRS) return "more than COEB_FUSE_MAX_PAIRS points";
    *code = COEB_OK;
    *total = sum;
    return nullptr;
}

void kfdb_fuse_pack(const coeb_fuse_job* jobs, int njobs, const KfdbGridRec* rec, const coeb_camera* cam,
                    std::vector<KfdbFuseJob>& tab, std::vector<uint8_t>& skip, std::vector<int32_t>& build)
{
    tab.assign((size_t)njobs, KfdbFuseJob{});
    build.clear();
    size_t bytes = 0;
    int32_t out = 0;
    for (int j = 0; j < njobs; j++) {
        const coeb_fuse_job& b = jobs[j];
        KfdbFuseJob& t = tab[j];
        t.slot = b.slot; t.first = b.first; t.count = b.count; t.out_off = out; t.skip_off = -1;
        std::copy(b.Rcw, b.Rcw + 9, t.Rcw);
        std::copy(b.tcw, b.tcw + 3, t.tcw);
        std::copy(b.Ow, b.Ow + 3, t.Ow);
        out += b.count;
        if (b.skip && b.count) {
            t.skip_off = (int32_t)bytes;
            bytes += ((size_t)b.count + 15) & ~(size_t)15;
        }
        if (b.count && !kfdb_grid_current(rec[b.slot], cam)) build.push_back(b.slot);
    }
    std::sort(build.begin(), build.end());
    build.erase(std::unique(build.begin(), build.end()), build.end());
    skip.assign(bytes, 0);
    for (int j = 0; j < njobs; j++)
        if (tab[j].skip_off >= 0) std::copy(jobs[j].skip, jobs[j].skip + jobs[j].count, skip.begin() + tab[j].skip_off);
}

// ---- CreateNewMapPoints over stored keyframes: the stereo records and argument rules ----
bool kfdb_pack_stereo(const float* key_xy, const float* depth, int n, KfdbStereo* out, uint8_t* depth_pos)
{
    for (int i = 0; i < n; i++) {
        const float x = key_xy[2 * i], y = key_xy[2 * i + 1], d = depth[i];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(d)) return false;
        out[i] = KfdbStereo{x, y, d, 0.f};
        depth_pos[i] = d > 0.0f;
    }
    return true;
}

bool kfdb_stereo_conflict(const uint8_t* is_stereo, const uint8_t* depth_pos, int n)
{
    for (int i = 0; i < n; i++)
        if (is_stereo[i] && !depth_pos[i]) return true;
    return false;
}

static bool view_finite(const coeb_kf_view& v)
{
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(v.Rcw[k])) return false;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(v.tcw[k]) || !std::isfinite(v.Ow[k])) return false;
    const float cam[8] = {v.fx, v.fy, v.cx, v.cy, v.invfx, v.invfy, v.mb, v.mbf};
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(cam[k])) return false;
    return true;
}

const char* kfdb_newpts_check(const uint8_t* used, const uint8_t* geo, const uint8_t* stereo, const uint8_t* conflict,
                              const int* n, int nslots, int slot1, const coeb_kf_view* view1, const uint8_t* has_mp1,
                              const int32_t* slots2, int nnb, const coeb_kf_view* views2, const uint8_t* const* has_mp2,
                              const float* F12, const float* epipole, const int32_t* match_out, const int8_t* status,
                              const float* x3d, const int32_t* first_ok, const int32_t* nmatches)
{
    if (const char* why = kfdb_tri_check(used, geo, n, nslots, slot1, has_mp1, slots2, nnb, has_mp2, F12, epipole, match_out,
                                         nmatches))
        return why;
    if (!stereo[slot1]) return "slot1 has no stereo data (coeb_kfdb_set_stereo)";
    if (conflict[slot1]) return "slot1 has a feature with u_right >= 0 and depth <= 0";
    if (!view1) return "missing view of keyframe 1";
    if (!view_finite(*view1)) return "a pose or camera entry of keyframe 1 is not finite";
    if (n[slot1] && !first_ok) return "missing first_ok";
    if (nnb == 0) return nullptr;
    if (!views2) return "missing views of the neighbours";
    if (n[slot1] && (!status || !x3d)) return "missing status or x3d";
    for (int j = 0; j < nnb; j++) {
        const int s = slots2[j];
        if (s == slot1) return "a neighbour is keyframe 1 itself";
        for (int k = 0; k < j; k++)
            if (slots2[k] == s) return "a neighbour's slot is repeated";
        if (!stereo[s]) return "a neighbour's slot has no stereo data (coeb_kfdb_set_stereo)";
        if (conflict[s]) return "a neighbour has a feature with u_right >= 0 and depth <= 0";
        if (!view_finite(views2[j])) return "a pose or camera entry of a neighbour is not finite";
    }
    return nullptr;
}

void kfdb_newpts_unpack(const int32_t* match, const int8_t* status, const float* x3d_dev, const int32_t* first_dev,
                        int nnb, int n1, float* x3d, int32_t* first_ok, int32_t* nmatches)
{
    for (int j = 0; j < nnb; j++) {
        int nm = 0;
        for (int i = 0; i < n1; i++) {
            const size_t e = (size_t)j * n1 + i;
            nm += match[e] >= 0;
            if ((status[e] & 15) == kNpAccepted)
                for (int k = 0; k < 3; k++) x3d[3 * e + k] = x3d_dev[3 * e + k];
        }
        nmatches[j] = nm;
    }
    for (int i = 0; i < n1; i++) first_ok[i] = first_dev[i] >= nnb ? -1 : first_dev[i];
}
