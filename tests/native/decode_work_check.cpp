// TEST INFRASTRUCTURE: welle.io_amd/csrc/decode_work.h compiled for the host.  Work items round-trip at both limits; the history
// geometry equals the literal formulas the host side carried before the header existed, for every code word length there is
// (24 * bitrate + 6 trellis steps at 8 .. 384 kbit/s in steps of 8, and the FIC's 774).  Prints one JSON line.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "decode_work.h"
using namespace dabphy;
int main() {
    long item_errors = 0, items = 0;
    const uint32_t classes[] = {0, 1, WORK_MAX_CLASSES - 1, WORK_MAX_CLASSES}, groups[] = {0, 1, 63, 64, WORK_MAX_GROUPS - 1, WORK_MAX_GROUPS};
    for (uint32_t c : classes) for (uint32_t g : groups) {
        const uint32_t wk = work_item(c, g);
        items++;
        if (work_class(wk) != c || work_group(wk) != g || wk != ((c << 24) | g)) item_errors++;
    }
    long geometry_errors = 0, lengths = 0;
    auto check = [&](size_t nsteps) {
        lengths++;
        if (hist_rows(nsteps) != nsteps / 30 + 1 || hist_cells(nsteps, false) != (nsteps / 30 + 1) * 32 || hist_cells(nsteps, true) != (nsteps / 30 + 1) * 64) geometry_errors++;
    };
    for (int bitrate = 8; bitrate <= 384; bitrate += 8) check((size_t)24 * bitrate + 6);
    check(774);
    printf("{\"items\": %ld, \"item_errors\": %ld, \"lengths\": %ld, \"geometry_errors\": %ld, \"hist_steps\": %d, \"max_classes\": %u, \"max_groups\": %u}\n",
           items, item_errors, lengths, geometry_errors, HIST_STEPS, WORK_MAX_CLASSES, WORK_MAX_GROUPS);
    return item_errors || geometry_errors ? 1 : 0;
}
