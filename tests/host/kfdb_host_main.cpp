// The host half of the keyframe database (csrc/coeb_kfdb_host.cpp) as a stand-alone program, built
// under ASan + UBSan by tests/test_kfdb_ref.py (no Python process, no GPU, no HIP).
//
//   kfdb_host FILE...
//
// Every FILE is one coeb_bow_vector case written by the test: int32 {n, normalize_l1, cap,
// expected rc, expected nw}, then word[n] i32, node[n] i32, weight[n] f64 and the expected
// word[nw] i32 / value[nw] f64 (present when rc is 0).  Values must agree bit for bit.  The list
// order and the word threshold of DetectRelocalizationCandidates are checked on literals.
#include <cstdio>
#include <cstring>
#include <vector>

#include "coeb_front.h"
#include "coeb_kfdb_host.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } \
    } while (0)

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int bow_case(const char* path)
{
    FILE* f = fopen(path, "rb");
    CHECK(f);
    std::vector<int32_t> hdr, word, node, want_word;
    std::vector<double> weight, want_value;
    CHECK(rd(f, hdr, 5));
    const int n = hdr[0], norm = hdr[1], cap = hdr[2], want_rc = hdr[3], want_nw = hdr[4];
    CHECK(n >= 0 && cap >= 0 && want_nw >= 0);
    CHECK(rd(f, word, n) && rd(f, node, n) && rd(f, weight, n));
    if (want_rc == 0) CHECK(rd(f, want_word, want_nw) && rd(f, want_value, want_nw));
    fclose(f);
    // exactly cap entries: a write past them is a heap overflow the sanitizer reports
    std::vector<int32_t> w_out((size_t)cap);
    std::vector<double> v_out((size_t)cap);
    int nw = -1;
    const int rc = coeb_bow_vector(n ? word.data() : nullptr, n ? weight.data() : nullptr, n ? node.data() : nullptr, n,
                                   norm, cap ? w_out.data() : nullptr, cap ? v_out.data() : nullptr, cap, &nw);
    CHECK(rc == want_rc);
    CHECK(nw == want_nw);
    if (rc == 0 && nw) {
        CHECK(memcmp(w_out.data(), want_word.data(), (size_t)nw * 4) == 0);
        CHECK(memcmp(v_out.data(), want_value.data(), (size_t)nw * 8) == 0);
    }
    return 0;
}

static int list_order()
{
    // slots 0..5; 1 and 4 share the first word 3: the earlier insertion (slot 4, seq 2) comes first
    const int32_t common[6] = {2, 1, 0, 5, 3, 1};
    const int32_t first[6] = {7, 3, 0x7fffffff, 9, 3, 1};
    const int64_t seq[6] = {0, 6, 1, 3, 2, 5};
    int32_t order[6];
    CHECK(kfdb_sharing_order(common, first, seq, 6, order) == 5);
    const int32_t want[5] = {5, 4, 1, 0, 3};
    CHECK(memcmp(order, want, sizeof(want)) == 0);
    CHECK(kfdb_sharing_order(common, first, seq, 0, order) == 0);
    // int minCommonWords = maxCommonWords * 0.8f
    CHECK(kfdb_min_common(0) == 0 && kfdb_min_common(1) == 0 && kfdb_min_common(3) == 2 && kfdb_min_common(5) == 4);
    CHECK(kfdb_min_common(10) == 8 && kfdb_min_common(137) == 109 && kfdb_min_common(4095) == 3276);
    const int32_t asc[4] = {0, 2, 3, 9}, eq[3] = {1, 1, 2}, desc[2] = {5, 4}, neg[2] = {-1, 4};
    CHECK(kfdb_words_ascending(asc, 4) && kfdb_words_ascending(nullptr, 0));
    CHECK(!kfdb_words_ascending(eq, 3) && !kfdb_words_ascending(desc, 2) && !kfdb_words_ascending(neg, 2));
    // argument checks of the entry point
    int nw = 0;
    CHECK(coeb_bow_vector(nullptr, nullptr, nullptr, -1, 1, nullptr, nullptr, 0, &nw) == COEB_EINVAL);
    CHECK(coeb_bow_vector(nullptr, nullptr, nullptr, 0, 1, nullptr, nullptr, 0, nullptr) == COEB_EINVAL);
    CHECK(coeb_bow_vector(nullptr, nullptr, nullptr, 3, 1, nullptr, nullptr, 0, &nw) == COEB_EINVAL);
    return 0;
}

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++)
        if (bow_case(argv[i])) { fprintf(stderr, "case %s failed\n", argv[i]); return 1; }
    if (list_order()) return 1;
    printf("ok\n");
    return 0;
}
