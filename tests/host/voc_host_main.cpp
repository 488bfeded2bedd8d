// The vocabulary parser (csrc/coeb_voc.cpp) as a stand-alone program for ASan + UBSan
// (tests/test_voc_host.py): voc_host_main FILE RC [FILE RC ...] parses every file from a heap
// buffer of exactly its size (no terminator: a read past the text is a sanitizer error) and
// compares the return code; a text that parses is walked through coeb_voc_info / coeb_voc_tables,
// and every prefix of it is parsed as well (a truncated file must give a code, never a crash).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coeb_front.h"

static int fail(const char* what, const char* file, int got)
{
    printf("FAIL %s: %s (%d)\n", what, file, got);
    return 1;
}

static int parse(const char* text, size_t len, coeb_voc** voc)
{
    char* buf = static_cast<char*>(malloc(len ? len : 1));
    if (len) memcpy(buf, text, len);
    const int rc = coeb_voc_from_text(buf, len, voc);
    free(buf);
    return rc;
}

int main(int argc, char** argv)
{
    for (int a = 1; a + 1 < argc; a += 2) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return fail("open", argv[a], 0);
        std::vector<char> text;
        char chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) text.insert(text.end(), chunk, chunk + got);
        fclose(f);
        const int want = atoi(argv[a + 1]);
        coeb_voc* voc = nullptr;
        const int rc = parse(text.data(), text.size(), &voc);
        if (rc != want) return fail("return code", argv[a], rc);
        if (rc != COEB_OK) {
            if (voc) return fail("handle set on failure", argv[a], rc);
            continue;
        }
        int k, L, nn, nw;
        if (coeb_voc_info(voc, &k, &L, &nn, &nw) != COEB_OK || nn < 2 || nw < 1) return fail("info", argv[a], nn);
        std::vector<int32_t> first(nn), count(nn), word(nn), id(nn), wnode(nw);
        std::vector<uint8_t> pos(nn), desc((size_t)nn * 32);
        std::vector<double> ww(nw);
        if (coeb_voc_tables(voc, first.data(), count.data(), word.data(), id.data(), pos.data(), desc.data(), ww.data(),
                            wnode.data()) != COEB_OK)
            return fail("tables", argv[a], 0);
        int words = 0;
        for (int s = 0; s < nn; s++) {
            if (count[s] < 0 || count[s] > k || (count[s] && (first[s] <= s || first[s] + count[s] > nn)))
                return fail("children range", argv[a], s);
            if ((count[s] == 0) != (word[s] >= 0)) return fail("word of inner node", argv[a], s);
            words += word[s] >= 0;
        }
        if (words != nw) return fail("word count", argv[a], words);
        coeb_voc_destroy(voc);
        for (size_t cut = 0; cut < text.size(); cut += (text.size() > 20000 ? 97 : 1)) {
            coeb_voc* v2 = nullptr;
            const int r2 = parse(text.data(), cut, &v2);
            if (r2 != COEB_OK && r2 != COEB_EINVAL) return fail("prefix code", argv[a], r2);
            if ((r2 == COEB_OK) != (v2 != nullptr)) return fail("prefix handle", argv[a], r2);
            coeb_voc_destroy(v2);
        }
    }
    coeb_voc* v = nullptr;
    if (coeb_voc_from_text(nullptr, 0, &v) != COEB_EINVAL) return fail("null text", "-", 0);
    coeb_voc_destroy(nullptr);
    printf("ok\n");
    return 0;
}
