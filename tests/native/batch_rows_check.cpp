// TEST INFRASTRUCTURE: welle.io_amd/csrc/batch_rows.h compiled for the host.  The first row a pair emits in a batch equals what the
// kernels and the host getter each computed before the header existed -- the kernels' loop (clamped to n_rows) and the host's expression
// (not clamped) -- for every distance between the batch's first CIF and the pair's cif0 around the 16-CIF fill and every row count of
// a batch; the layout of the filter's carried window is asserted at compile time.  Prints one JSON line.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "batch_rows.h"
using namespace dabphy;

static_assert(TDI_FILL_CIFS == 16 && SF_STATE_HEAD == 16, "16 CIFs of fill; 16 bytes in front of the frames");
static_assert(sf_state_stride(24) == 144 && sf_state_stride(192) == 976 && sf_state_stride(1152) == 5776, "16 + 5 frames, rounded up to 16: 8, 64 and 384 kbit/s");

int main() {
    long cases = 0, errors = 0;
    const int64_t frame_nos[] = {0, 1, 5, 1000003};
    for (int64_t frame_no : frame_nos)
        for (int d = -4; d <= 40; d++) {                                  // d = c0 - cif0
            const long long c0 = 4 * frame_no, cif0 = c0 - d;
            const int64_t first = batch_first_row(frame_no, cif0);
            const int64_t fed = c0 - cif0;                                // the host getter, as it was
            if (first != (fed >= 16 ? 0 : (int32_t)(16 - fed))) errors++;
            for (int n_rows = 0; n_rows <= 24; n_rows = n_rows ? n_rows + 4 : 4) {
                int r_first = 0;                                          // the kernels, as they were
                while (r_first < n_rows && c0 + r_first - cif0 < 16) r_first++;
                cases++;
                if ((first < n_rows ? (int)first : n_rows) != r_first) errors++;
                for (int r = 0; r < n_rows; r++)                          // ... and k_chanber's test of one row
                    if ((r >= first) != (c0 + r - cif0 >= 16)) errors++;
            }
        }
    uint8_t st[32] = {0};
    sf_state_count(st) = 3;
    if (st[0] != 3 || sf_state_count(st) != 3 || sf_state_frames(st) != st + 16) errors++;
    printf("{\"cases\": %ld, \"errors\": %ld}\n", cases, errors);
    return errors ? 1 : 0;
}
