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
