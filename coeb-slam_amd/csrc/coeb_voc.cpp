// The bag-of-words vocabulary on the host (C++, no device code).
//
// Replaces what the tracking thread needs of DBoW2's TemplatedVocabulary<ORB>: loadFromTextFile
// as ORB-SLAM2 ships it (ORBvoc.txt) and the tree the transform walks.  Written from the format,
// not from DBoW2 (absent here; parity against it is UNPINNED):
//   * the first line is "k L scoring weighting";
//   * every further non-empty line is "parent is_leaf d0 .. d31 weight" and defines the next node
//     id (1, 2, ..; 0 is the root); it is appended to its parent's children; leaves take the word
//     ids 0, 1, .. in line order.
// A file DBoW2 would read into an inconsistent tree is refused: a parent that is not defined yet
// or is itself a leaf, more than k children, a node below level L, an inner node without children.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <locale.h>
#include <memory>
#include <new>
#include <stdlib.h>

#include "../../include/coeb_front.h"
#include "coeb_voc.hpp"

namespace {

// Tokens of one text, separated by blanks; a line ends at '\n'.
struct Scan {
    const char* t;
    size_t i, e;
    void blanks() { while (i < e && (t[i] == ' ' || t[i] == '\t' || t[i] == '\r')) i++; }
    bool eol() { blanks(); return i >= e || t[i] == '\n'; }
    // the next token of the line as [b, b + n); false at the end of the line
    bool token(const char** b, size_t* n)
    {
        if (eol()) return false;
        const size_t s = i;
        while (i < e && t[i] != ' ' && t[i] != '\t' && t[i] != '\r' && t[i] != '\n') i++;
        *b = t + s;
        *n = i - s;
        return true;
    }
    bool integer(long lo, long hi, long* v)
    {
        const char* b;
        size_t n;
        if (!token(&b, &n) || n > 10) return false;
        size_t j = 0;
        const bool neg = b[0] == '-';
        if (neg) j++;
        if (j >= n) return false;
        long x = 0;
        for (; j < n; j++) {
            if (b[j] < '0' || b[j] > '9') return false;
            x = x * 10 + (b[j] - '0');
        }
        if (neg) x = -x;
        if (x < lo || x > hi) return false;
        *v = x;
        return true;
    }
    bool real(double* v)
    {
        const char* b;
        size_t n;
        char buf[64];
        if (!token(&b, &n) || n >= sizeof buf) return false;
        memcpy(buf, b, n);
        buf[n] = 0;
        static const locale_t loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
        char* end = nullptr;
        *v = strtod_l(buf, &end, loc);
        return end == buf + n;
    }
    void next_line() { if (i < e) i++; }      // past the '\n' eol() stopped at
};

// node i + 1 = (parent[i], is_leaf[i], desc[i], weight[i]) for i < n
int build(int k, int L, int scoring, int weighting, int64_t n, const int32_t* parent, const uint8_t* is_leaf,
          const uint8_t* desc, const double* weight, coeb_voc** out)
{
    if (k < 2 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
        return COEB_EINVAL;
    if (n < 1 || n >= (int64_t)1 << 30) return COEB_EINVAL;
    const int nn = (int)n + 1;
    std::vector<int32_t> count(nn, 0), depth(nn, 0), first(nn, 0);
    for (int i = 1; i < nn; i++) {
        const int p = parent[i - 1];
        if (p < 0 || p >= i) return COEB_EINVAL;                 // not a node already defined
        if (p > 0 && is_leaf[p - 1]) return COEB_EINVAL;
        if (++count[p] > k) return COEB_EINVAL;
        depth[i] = depth[p] + 1;
        if (depth[i] > L) return COEB_EINVAL;
    }
    for (int i = 1; i < nn; i++)
        if ((count[i] == 0) != (is_leaf[i - 1] != 0)) return COEB_EINVAL;
    std::unique_ptr<coeb_voc> v(new coeb_voc());
    v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting; v->nnodes = nn;
    // slots breadth first: a node's children take the next count[node] slots, in line order
    v->slot_of.assign(nn, 0);
    std::vector<int32_t> node_of(nn, 0), fill(nn, 0);
    {
        // children of p in line order = ascending node id: bucket them
        std::vector<int32_t> cstart(nn + 1, 0), child(nn > 1 ? nn - 1 : 0);
        for (int p = 0; p < nn; p++) cstart[p + 1] = cstart[p] + count[p];
        for (int i = 1; i < nn; i++) child[cstart[parent[i - 1]] + fill[parent[i - 1]]++] = i;
        int next = 1;
        for (int s = 0; s < nn; s++) {                           // node_of[s] is set before s is reached
            const int p = node_of[s];
            first[p] = next;
            for (int c = 0; c < count[p]; c++) {
                const int id = child[cstart[p] + c];
                node_of[next] = id;
                v->slot_of[id] = next++;
            }
        }
    }
    v->rec.resize(nn);
    v->desc.assign((size_t)nn * 32, 0);
    for (int i = 1; i < nn; i++)
        if (is_leaf[i - 1]) {
            v->word_weight.push_back(weight[i - 1]);
            v->word_node.push_back(i);
        }
    v->nwords = (int)v->word_weight.size();
    int word = 0;
    std::vector<int32_t> word_of(nn, -1);
    for (int i = 1; i < nn; i++)
        if (is_leaf[i - 1]) word_of[i] = word++;
    for (int s = 0; s < nn; s++) {
        const int id = node_of[s];
        VocRec& r = v->rec[s];
        r.child_first = count[id] ? first[id] : 0;
        r.child_count = count[id];
        r.word = word_of[id];
        r.id_flag = (uint32_t)id;
        if (id > 0) {
            if (is_leaf[id - 1] && weight[id - 1] > 0) r.id_flag |= kVocPositive;
            memcpy(&v->desc[(size_t)s * 32], desc + (size_t)(id - 1) * 32, 32);
        }
    }
    *out = v.release();
    return COEB_OK;
}

}  // namespace

extern "C" {

int coeb_voc_from_text(const char* text, size_t len, coeb_voc** voc)
{
    if (!text || !voc) return COEB_EINVAL;
    *voc = nullptr;
    try {
    Scan sc{text, 0, len};
    while (sc.i < len && sc.eol()) sc.next_line();               // leading empty lines
    long k, L, scoring, weighting;
    if (!sc.integer(2, 20, &k) || !sc.integer(1, 10, &L) || !sc.integer(0, 5, &scoring) || !sc.integer(0, 3, &weighting) ||
        !sc.eol())
        return COEB_EINVAL;
    sc.next_line();
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf, desc;
    std::vector<double> weight;
    while (sc.i < len) {
        if (sc.eol()) { sc.next_line(); continue; }
        long p, lf, b;
        if (!sc.integer(0, (long)parent.size(), &p) || !sc.integer(0, 0x7fffffff, &lf)) return COEB_EINVAL;
        parent.push_back((int32_t)p);
        leaf.push_back(lf > 0);
        for (int j = 0; j < 32; j++) {
            if (!sc.integer(0, 255, &b)) return COEB_EINVAL;
            desc.push_back((uint8_t)b);
        }
        double w;
        if (!sc.real(&w) || !sc.eol()) return COEB_EINVAL;
        weight.push_back(w);
        sc.next_line();
    }
    if (parent.empty()) return COEB_EINVAL;
    return build((int)k, (int)L, (int)scoring, (int)weighting, (int64_t)parent.size(), parent.data(), leaf.data(),
                 desc.data(), weight.data(), voc);
    } catch (const std::bad_alloc&) {
        return COEB_ENOMEM;
    }
}

int coeb_voc_from_arrays(int k, int L, int nlines, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                         const double* weight, coeb_voc** voc)
{
    if (!voc) return COEB_EINVAL;
    *voc = nullptr;
    if (nlines < 1 || !parent || !is_leaf || !desc || !weight) return COEB_EINVAL;
    try {
        return build(k, L, 0, 0, nlines, parent, is_leaf, desc, weight, voc);
    } catch (const std::bad_alloc&) {
        return COEB_ENOMEM;
    }
}

int coeb_voc_info(const coeb_voc* voc, int* k, int* L, int* nnodes, int* nwords)
{
    if (!voc) return COEB_EINVAL;
    if (k) *k = voc->k;
    if (L) *L = voc->L;
    if (nnodes) *nnodes = voc->nnodes;
    if (nwords) *nwords = voc->nwords;
    return COEB_OK;
}

int coeb_voc_tables(const coeb_voc* voc, int32_t* child_first, int32_t* child_count, int32_t* word, int32_t* node_id,
                    uint8_t* positive, uint8_t* desc, double* word_weight, int32_t* word_node)
{
    if (!voc) return COEB_EINVAL;
    for (int s = 0; s < voc->nnodes; s++) {
        const VocRec& r = voc->rec[s];
        if (child_first) child_first[s] = r.child_first;
        if (child_count) child_count[s] = r.child_count;
        if (word) word[s] = r.word;
        if (node_id) node_id[s] = (int32_t)(r.id_flag & ~kVocPositive);
        if (positive) positive[s] = (r.id_flag & kVocPositive) != 0;
    }
    if (desc) memcpy(desc, voc->desc.data(), voc->desc.size());
    for (int w = 0; w < voc->nwords; w++) {
        if (word_weight) word_weight[w] = voc->word_weight[w];
        if (word_node) word_node[w] = voc->word_node[w];
    }
    return COEB_OK;
}

void coeb_voc_destroy(coeb_voc* voc) { delete voc; }

}  // extern "C"
