// The rules about byte ranges that the argument checks of the entry points share: whether two ranges share a byte, the
// bytes a strided column spans, and "no output may overlap an input or another output" over a table of ranges.  Plain
// C++, nothing of HIP: a host program can include this file alone (tests/test_argrules.py does).  The messages of a
// refused call stay with the check that refuses it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace gridhip {

// do the abytes at a and the bbytes at b share a byte?  Never for a null pointer or an empty range.
static inline bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}

// the bytes from the first to the last of n items of `width` doubles each, `stride` doubles apart
static inline size_t span_bytes(int64_t n, int64_t stride, int64_t width = 1)
{
    return n > 0 ? ((size_t)(n - 1) * (size_t)stride + (size_t)width) * 8 : 0;
}

struct Range {
    const void *p;
    size_t bytes;
};

static inline bool overlaps_any(Range r, std::initializer_list<Range> list)
{
    for (const Range &o : list)
        if (overlap(r.p, r.bytes, o.p, o.bytes)) return true;
    return false;
}

// An output that may be one of the inputs itself (the in-place forms): outs[out].p == ins[in].p is then no clash.
struct InPlace {
    int out, in;
};
// Each output against every input, then against every later output.  0: no two overlap; 1: an output overlaps an input
// (other than as `same` allows); 2: two outputs overlap.
static inline int outputs_clash(std::initializer_list<Range> outs, std::initializer_list<Range> ins,
                                std::initializer_list<InPlace> same = {})
{
    const Range *o = outs.begin(), *i = ins.begin();
    for (int a = 0; a < (int)outs.size(); ++a) {
        for (int b = 0; b < (int)ins.size(); ++b) {
            bool allowed = false;
            for (const InPlace &s : same) allowed = allowed || (s.out == a && s.in == b && o[a].p == i[b].p);
            if (!allowed && overlap(o[a].p, o[a].bytes, i[b].p, i[b].bytes)) return 1;
        }
        for (int q = a + 1; q < (int)outs.size(); ++q)
            if (overlap(o[a].p, o[a].bytes, o[q].p, o[q].bytes)) return 2;
    }
    return 0;
}

}  // namespace gridhip
