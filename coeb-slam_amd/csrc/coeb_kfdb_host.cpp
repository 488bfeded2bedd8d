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
