// bin_digest_check - the pre-record digest of the binning pre-pass (csrc/bin_digest.h) as a program of its own:
// tests/test_bin_digest_host.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <vector>

#include "../csrc/bin_digest.h"

using namespace gridhip;

static int failures = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static uint64_t rnd(uint64_t *s)
{
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return *s ^ (*s >> 29);
}
static bool same(const Digest &x, const Digest &y) { return x.a == y.a && x.b == y.b; }

int main()
{
    uint64_t seed = 12345;
    // any single bit of a pre-record: both words of the element's contribution change (the mixes are bijections)
    const uint64_t indices[] = {0, 1, 63, 64, 127, 128, 16384, (1ull << 31) - 1, (1ull << 31) + 5, 99999999};
    for (uint64_t index : indices) {
        for (int t = 0; t < 20; ++t) {
            // (a packed record of the headline case has 54 bits; all ones = dropped; zero = bin 0's first record)
            const uint64_t p = t == 0 ? 0 : t == 1 ? ~0ull : t == 2 ? rnd(&seed) & ((1ull << 54) - 1) : rnd(&seed);
            const Digest d = digest_elem(p, index);
            for (int bit = 0; bit < 64; ++bit) {
                const Digest f = digest_elem(p ^ (1ull << bit), index);
                EXPECT(f.a != d.a && f.b != d.b);
            }
            // the same pre-record at another place of the group contributes something else
            const Digest o = digest_elem(p, index ^ 1);
            EXPECT(o.a != d.a && o.b != d.b);
        }
    }
    // the salt is linear, as the sweeps that step it by addition assume
    for (int t = 0; t < 100; ++t) {
        const uint64_t i = rnd(&seed) >> 20, d = rnd(&seed) >> 30;
        EXPECT(digest_salt(i + d) == digest_salt(i) + digest_salt(d));
    }
    EXPECT(digest_salt(1) == DIGEST_SALT);

    // a group's digest is the wrapping sum of its elements' contributions, in any order
    const int64_t n = 3 * DIGEST_GROUP + 1;
    std::vector<uint64_t> pre((size_t)n);  // (exactly n long: a read past the end is the sanitizer's)
    for (auto &p : pre) p = rnd(&seed) & ((1ull << 54) - 1);
    pre[5] = ~0ull;
    for (int64_t grp = 0; grp < 4; ++grp) {
        Digest back{0, 0};
        for (int64_t i = (grp + 1) * DIGEST_GROUP - 1; i >= grp * DIGEST_GROUP; --i)
            if (i < n) digest_add(back, digest_elem(pre[(size_t)i], (uint64_t)i));
        EXPECT(same(digest_group(pre.data(), n, grp), back));
    }
    // two distinct pre-records that swap places inside a group change its digest; across groups, both groups' digests
    const int64_t pairs[][2] = {{0, 1}, {6, 7}, {0, 127}, {63, 64}, {126, 127}, {128, 255}, {130, 131}, {127, 128}, {255, 256}};
    for (const auto &pr : pairs) {
        const int64_t i = pr[0], j = pr[1];
        EXPECT(pre[(size_t)i] != pre[(size_t)j]);
        std::vector<uint64_t> sw(pre);
        sw[(size_t)i] = pre[(size_t)j];
        sw[(size_t)j] = pre[(size_t)i];
        for (int64_t grp = 0; grp < 4; ++grp) {
            const bool touched = grp == i / DIGEST_GROUP || grp == j / DIGEST_GROUP;
            const Digest x = digest_group(pre.data(), n, grp), y = digest_group(sw.data(), n, grp);
            EXPECT(touched ? (x.a != y.a && x.b != y.b) : same(x, y));
        }
    }
    // elements past n contribute nothing: the last group is its one element, a group beyond the end is zero
    EXPECT(same(digest_group(pre.data(), n, 3), digest_elem(pre[(size_t)n - 1], (uint64_t)n - 1)));
    EXPECT(same(digest_group(pre.data(), n, 4), Digest{0, 0}));
    EXPECT(same(digest_group(pre.data(), 3 * DIGEST_GROUP, 3), Digest{0, 0}));
    EXPECT(same(digest_group(pre.data(), 1, 0), digest_elem(pre[0], 0)));
    // a shorter stream with the same leading pre-records has another digest in the group it ends in, the same before
    EXPECT(same(digest_group(pre.data(), 200, 0), digest_group(pre.data(), n, 0)));
    EXPECT(!same(digest_group(pre.data(), 200, 1), digest_group(pre.data(), n, 1)));

    if (failures) return 1;
    printf("bin_digest ok\n");
    return 0;
}
