// argrules_check - the byte-range rules of the argument checks (csrc/argrules.h) on their edge cases, as a program of
// its own: tests/test_argrules.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <cstdio>

#include "../csrc/argrules.h"

using namespace gridhip;

static int failures = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

int main()
{
    static double buf[64];
    const char *b = reinterpret_cast<const char *>(buf);
    // overlap: null pointers, empty ranges
    EXPECT(!overlap(nullptr, 8, b, 8) && !overlap(b, 8, nullptr, 8) && !overlap(nullptr, 8, nullptr, 8));
    EXPECT(!overlap(b, 0, b, 8) && !overlap(b, 8, b, 0) && !overlap(b + 4, 0, b, 8));
    // identical ranges, containment either way
    EXPECT(overlap(b, 8, b, 8));
    EXPECT(overlap(b, 64, b + 16, 8) && overlap(b + 16, 8, b, 64));
    // one byte shared at either end
    EXPECT(overlap(b, 9, b + 8, 8) && overlap(b + 8, 8, b, 9));
    EXPECT(overlap(b + 15, 8, b + 8, 8) && overlap(b + 8, 8, b + 15, 8));
    // ranges that touch share nothing
    EXPECT(!overlap(b, 8, b + 8, 8) && !overlap(b + 8, 8, b, 8));

    // span_bytes: n = 0 and 1, strides 1 and 3, widths 1 and 2
    EXPECT(span_bytes(0, 1) == 0 && span_bytes(0, 3, 2) == 0 && span_bytes(-1, 3) == 0);
    EXPECT(span_bytes(1, 1) == 8 && span_bytes(1, 3) == 8 && span_bytes(1, 3, 2) == 16);
    EXPECT(span_bytes(5, 1) == 40 && span_bytes(5, 3) == 104 && span_bytes(5, 2, 2) == 80 && span_bytes(5, 3, 2) == 112);

    // the list helpers on a table of three ranges
    const Range x = {b, 16}, y = {b + 16, 16}, z = {b + 40, 8};
    EXPECT(!overlaps_any(x, {y, z}) && overlaps_any({b + 8, 16}, {z, y}) && !overlaps_any({nullptr, 16}, {x, y, z}));
    EXPECT(!overlaps_any(x, {}));
    EXPECT(outputs_clash({x, y}, {z}) == 0);
    EXPECT(outputs_clash({x, y}, {z, x}) == 1);            // an output that is an input, not allowed
    EXPECT(outputs_clash({x, y}, {z, x}, {{0, 1}}) == 0);  // the one allowed identical pair
    EXPECT(outputs_clash({x, y}, {z, x}, {{1, 1}}) == 1);  // allowed for another output only
    EXPECT(outputs_clash({{b + 8, 16}, y}, {z, x}, {{0, 1}}) == 1);  // overlapping, but not the input itself
    EXPECT(outputs_clash({x, y, {b + 24, 8}}, {z}) == 2);  // two outputs
    // output by output: the first one's later outputs come before the second one's inputs
    EXPECT(outputs_clash({x, {b + 8, 4}}, {x}, {{0, 0}}) == 2);
    EXPECT(outputs_clash({z, {b + 8, 4}}, {x}, {{0, 0}}) == 1);
    EXPECT(outputs_clash({x, {nullptr, 8}, {b + 60, 0}}, {{nullptr, 64}, z}) == 0);  // absent arguments clash with nothing
    if (failures == 0) printf("argrules ok\n");
    return failures == 0 ? 0 : 1;
}
