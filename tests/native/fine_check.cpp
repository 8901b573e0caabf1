// TEST INFRASTRUCTURE: host-side check of welle.io_amd/csrc/sync_fine.h (compiled with g++ against the hipemu header).
// Reads trials from the file named on the command line, each 1 + 37 800 + 37 800 float32 values: fine_old, the real parts and the
// imaginary parts of a frame's 75 x 504 cyclic-prefix products in index order.  Forms the block sums as sync_finish_body
// (k_sync.hip) does -- per block of FIN_BLOCK_ROWS rows of 504: sum re, sum im, sum |re|, sum |im| in double precision -- calls the
// real fine_decided and prints one line per trial: "<decided 0/1> <fine_new>".
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "sync_fine.h"
using namespace dabphy;

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: fine_check TRIALS.f32\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    constexpr int ROWS = 75, N = ROWS * T_G;
    std::vector<float> rec(1 + 2 * (size_t)N);
    while (fread(rec.data(), sizeof(float), rec.size(), f) == rec.size()) {
        const float *re = rec.data() + 1, *im = re + N;
        double blk[FIN_BLOCKS][4] = {};
        for (int i = 0; i < N; i++) {
            double* s = blk[(i / T_G) / FIN_BLOCK_ROWS];
            s[0] += (double)re[i]; s[1] += (double)im[i]; s[2] += fabs((double)re[i]); s[3] += fabs((double)im[i]);
        }
        int32_t fine_new = 0;
        const bool decided = fine_decided((int32_t)rec[0], blk, fine_new);
        printf("%d %d\n", decided ? 1 : 0, (int)fine_new);
    }
    fclose(f);
    return 0;
}
