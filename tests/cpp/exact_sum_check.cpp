// exact_sum_check.cpp — the exact-sum core (csrc/sp_exact_sum.h) alone, under the host compiler: tests/test_mean_cpu.py builds this
// with -fsanitize=address,undefined and compares what it prints with math.fsum.
// stdin: one list per line, its values as hexadecimal 64-bit patterns separated by blanks (an empty line is the empty list).
// stdout: per line the pattern of RN(exact sum) with the NaN and inf rule, or "invalid" for a list with a negative value.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sp_exact_sum.h"

int main()
{
    std::string line;
    std::vector<uint64_t> v;
    for (int c = getchar();; c = getchar()) {
        if (c != '\n' && c != EOF) {
            line.push_back((char)c);
            continue;
        }
        if (c == EOF && line.empty()) break;
        v.clear();
        const char *p = line.c_str();
        for (;;) {
            char *end = nullptr;
            const uint64_t b = strtoull(p, &end, 16);
            if (end == p) break;
            v.push_back(b);
            p = end;
        }
        uint64_t sum = 0;
        if (spx::exact_sum_bits(v.data(), v.size(), &sum)) printf("%016" PRIx64 "\n", sum);
        else printf("invalid\n");
        line.clear();
        if (c == EOF) break;
    }
    return 0;
}
