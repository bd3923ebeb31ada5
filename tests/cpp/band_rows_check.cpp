// band_rows_check.cpp — the band code of csrc/sp_geometry.cpp (sp_band_rows, spgeo::check_bands) alone, under the host compiler:
// tests/test_band_cpu.py builds this with -fsanitize=address,undefined and compares what it prints with tests/bandref.py.
// stdin, one question per line:
//   rows <n> <f_lo> <f_hi>          (the edges as strtod reads them: hexadecimal floats, inf, nan)
//   bands <n> <count> <y0> <y1> ... (2 * count rows)
// stdout, per line: "0 <y0> <y1>" or sp_band_rows's status; "ok" or "refused".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spectroplot_hip.h"
#include "sp_geometry.h"

int main()
{
    std::string line;
    for (int c = getchar();; c = getchar()) {
        if (c != '\n' && c != EOF) {
            line.push_back((char)c);
            continue;
        }
        if (c == EOF && line.empty()) break;
        const char *p = line.c_str();
        char *end = nullptr;
        if (!strncmp(p, "rows ", 5)) {
            const int32_t n = (int32_t)strtol(p + 5, &end, 10);
            const double lo = strtod(end, &end), hi = strtod(end, &end);
            int32_t y0 = -7, y1 = -7;
            const int rc = sp_band_rows(n, lo, hi, &y0, &y1);
            if (rc) printf("%d\n", rc);
            else printf("0 %d %d\n", (int)y0, (int)y1);
        } else if (!strncmp(p, "bands ", 6)) {
            const int32_t n = (int32_t)strtol(p + 6, &end, 10);
            const int32_t count = (int32_t)strtol(end, &end, 10);
            std::vector<int32_t> rows;   // exactly 2 * count values on the heap: a read past them is the sanitizer's to find
            for (int32_t k = 0; k < 2 * count; k++) rows.push_back((int32_t)strtol(end, &end, 10));
            printf("%s\n", spgeo::check_bands(n, rows.empty() ? nullptr : rows.data(), count) ? "refused" : "ok");
        } else {
            printf("?\n");
        }
        line.clear();
        if (c == EOF) break;
    }
    return 0;
}
