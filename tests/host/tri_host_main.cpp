// The host half of coeb_kfdb_set_geometry / coeb_kfdb_search_triangulation
// (csrc/coeb_kfdb_host.cpp: the geometry records, the argument rules, the packed masks and slot
// table) as a stand-alone program, built under ASan + UBSan by tests/test_adapter_tri.py (no Python
// process, no GPU, no HIP).  Every buffer has exactly the size the rules promise, so a read or
// write past it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coeb_front.h"
#include "coeb_kfdb_host.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } \
    } while (0)

static bool says(const char* msg, const char* part) { return msg && strstr(msg, part); }

static int geometry()
{
    std::vector<coeb_keypoint> keys(5);
    std::vector<float> ur(5);
    for (int i = 0; i < 5; i++) {
        keys[i] = coeb_keypoint{1.5f * i, 2.0f + i, 31.f, 90.f, 0.f, i, -1};
        ur[i] = i & 1 ? -1.f : 0.25f * i;
    }
    std::vector<KfdbGeo> out(5);
    CHECK(kfdb_pack_geometry(keys.data(), ur.data(), 5, 8, out.data()));
    for (int i = 0; i < 5; i++)
        CHECK(out[i].x == keys[i].x && out[i].y == keys[i].y && out[i].u_right == ur[i] && out[i].octave == i);
    CHECK(!kfdb_pack_geometry(keys.data(), ur.data(), 5, 4, out.data()));       // octave 4 of a 4-level pyramid
    CHECK(kfdb_pack_geometry(keys.data(), ur.data(), 4, 4, out.data()));
    keys[2].octave = -1;
    CHECK(!kfdb_pack_geometry(keys.data(), ur.data(), 5, 8, out.data()));
    CHECK(kfdb_pack_geometry(nullptr, nullptr, 0, 8, nullptr));
    return 0;
}

static int rules()
{
    // slots: 0 (3 features, geometry), 1 (no features, geometry), 2 (2 features, no geometry), 3 empty
    const std::vector<uint8_t> used = {1, 1, 1, 0}, geo = {1, 1, 0, 0};
    const std::vector<int> n = {3, 0, 2, 0};
    const std::vector<uint8_t> m0(3), m2(2);
    std::vector<float> F(33 * 9), e(33 * 2);
    std::vector<int32_t> match(33 * 3), nm(33);
    std::vector<int32_t> slots = {0, 1, 0};
    std::vector<const uint8_t*> has = {m0.data(), nullptr, m0.data()};
    auto check = [&](int slot1, const uint8_t* h1, const int32_t* s2, int nnb, const uint8_t* const* h2, const float* f,
                     const float* ep, const int32_t* mo, const int32_t* cnt) {
        return kfdb_tri_check(used.data(), geo.data(), n.data(), 4, slot1, h1, s2, nnb, h2, f, ep, mo, cnt);
    };
    CHECK(!check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()));
    CHECK(!check(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));                 // nnb == 0
    CHECK(!check(1, nullptr, slots.data(), 3, has.data(), F.data(), e.data(), nullptr, nm.data()));     // n1 == 0
    CHECK(says(check(0, m0.data(), slots.data(), 33, has.data(), F.data(), e.data(), match.data(), nm.data()), "0..32"));
    CHECK(says(check(0, m0.data(), slots.data(), -1, has.data(), F.data(), e.data(), match.data(), nm.data()), "0..32"));
    CHECK(says(check(3, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "no keyframe"));
    CHECK(says(check(4, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "no keyframe"));
    CHECK(says(check(-1, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "no keyframe"));
    CHECK(says(check(2, m2.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "geometry"));
    CHECK(says(check(0, nullptr, slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), nullptr, nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), nullptr, 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), slots.data(), 3, nullptr, F.data(), e.data(), match.data(), nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), nullptr, e.data(), match.data(), nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), nullptr, match.data(), nm.data()), "missing"));
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nullptr), "missing"));
    slots[2] = 2;
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "geometry"));
    slots[2] = 3;
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "no keyframe"));
    slots[2] = 7;
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "no keyframe"));
    slots[2] = 0;
    has[2] = nullptr;
    CHECK(says(check(0, m0.data(), slots.data(), 3, has.data(), F.data(), e.data(), match.data(), nm.data()), "has_mp2"));
    return 0;
}

static int packing()
{
    // keyframes of 17, 0, 16 and 1 features; 32 neighbours cycle over them
    const std::vector<int> n = {17, 0, 16, 1};
    std::vector<std::vector<uint8_t>> mask(4);
    for (int s = 0; s < 4; s++)
        for (int i = 0; i < n[s]; i++) mask[s].push_back((uint8_t)((s * 31 + i * 7) % 3 == 0));
    std::vector<int32_t> slots;
    std::vector<const uint8_t*> has;
    for (int j = 0; j < 32; j++) {
        slots.push_back(j % 4);
        has.push_back(mask[j % 4].empty() ? nullptr : mask[j % 4].data());
    }
    std::vector<uint8_t> masks;
    std::vector<int32_t> tab;
    kfdb_tri_pack(n.data(), slots.data(), 32, has.data(), masks, tab);
    CHECK(tab.size() == 64 && masks.size() == 8 * (32 + 0 + 16 + 16));
    for (int j = 0; j < 32; j++) {
        const int s = j % 4, off = tab[2 * j + 1];
        CHECK(tab[2 * j] == s && off % 16 == 0 && off + n[s] <= (int)masks.size());
        CHECK(j == 0 || off >= tab[2 * j - 1] + n[slots[j - 1]]);
        CHECK(n[s] == 0 || memcmp(masks.data() + off, mask[s].data(), (size_t)n[s]) == 0);
    }
    kfdb_tri_pack(n.data(), slots.data(), 0, has.data(), masks, tab);
    CHECK(tab.empty() && masks.empty());
    const int32_t only_empty[2] = {1, 1};
    const uint8_t* none[2] = {nullptr, nullptr};
    kfdb_tri_pack(n.data(), only_empty, 2, none, masks, tab);
    CHECK(tab.size() == 4 && masks.empty() && tab[1] == 0 && tab[3] == 0);
    return 0;
}

int main()
{
    if (geometry() || rules() || packing()) return 1;
    printf("ok\n");
    return 0;
}
