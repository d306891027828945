// Digest of the binning pre-pass's pre-records (bin.hip, "Reuse"): plain C++, shared by the kernels and by a host
// program (host/bin_digest_check.cpp), so it includes nothing of HIP.
//
// The sweep's index space is cut into aligned groups of DIGEST_GROUP consecutive elements (group = index / 128: fixed
// by the index alone, whatever the launch shape).  Every element contributes two 64-bit words, two different
// splitmix-style finalisers (both bijections of the 64-bit word) of pre-record ^ salt(index); a group's digest is the
// wrapping sum of its elements' contributions, word by word.  Elements past the stream's end contribute nothing.
// The salt ties a pre-record to its place: two visibilities of one group that swap their coordinates change the sum.
//
// What equality means: the verify sweep compares 128-bit sums where it used to compare the pre-records themselves.  A
// single changed pre-record always changes its group's digest (the mixes are bijections); several changed ones leave it
// as it was only if the differences of their contributions cancel in both words, for mixes that behave like random
// functions with probability about 2^-128 per changed group - far below the rate of undetected memory errors.  Sums of
// digests are digests of the union of their groups (every term carries its index), so a sweep may add up the groups it
// has been through and compare once.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GH_DIGEST_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GH_DIGEST_FN inline
#endif

namespace gridhip {

constexpr int DIGEST_GROUP = 128;
struct Digest {
    uint64_t a, b;
};
static_assert(sizeof(Digest) == 16, "one 128-bit word per group");

// linear in the index (wrapping), so a loop may step it by addition: salt(i + d) = salt(i) + salt(d)
constexpr uint64_t DIGEST_SALT = 0x9e3779b97f4a7c15ull;
GH_DIGEST_FN uint64_t digest_salt(uint64_t index) { return index * DIGEST_SALT; }

GH_DIGEST_FN uint64_t digest_mix_a(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
GH_DIGEST_FN uint64_t digest_mix_b(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// one element's contribution, from its pre-record and its index's salt
GH_DIGEST_FN Digest digest_salted(uint64_t pre, uint64_t salt)
{
    const uint64_t x = pre ^ salt;
    return Digest{digest_mix_a(x), digest_mix_b(x)};
}
GH_DIGEST_FN Digest digest_elem(uint64_t pre, uint64_t index) { return digest_salted(pre, digest_salt(index)); }
GH_DIGEST_FN void digest_add(Digest &d, const Digest &e)
{
    d.a += e.a;
    d.b += e.b;
}

// the digest of group `group` of pre[0 .. n) (host reference of what the counting sweep stores)
inline Digest digest_group(const uint64_t *pre, int64_t n, int64_t group)
{
    Digest d{0, 0};
    for (int64_t i = group * DIGEST_GROUP; i < (group + 1) * DIGEST_GROUP && i < n; ++i) digest_add(d, digest_elem(pre[i], (uint64_t)i));
    return d;
}

}  // namespace gridhip
