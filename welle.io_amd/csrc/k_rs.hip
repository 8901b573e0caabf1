// welle.io_amd/csrc/k_rs.hip -- the bare Reed-Solomon seams: RS(120,110) (rs_codec.h) over superframes, one thread per codeword.
//
// Replaces (reference file:line):
//   RSDecoder::DecodeSuperframe          src/backend/dabplus_decoder.cpp:326-359
//
// A superframe of a sub-channel with s = bitrate/8 holds s column-interleaved codewords: codeword i consists of
// bytes sf[pos*s + i], pos = 0..119.  Consecutive threads take consecutive i, so every syndrome step reads s
// consecutive bytes.  The DAB+ superframe filter on the class output of a batch is k_superframe.hip.
#include "rs_codec.h"

namespace dabphy {

// Contiguous superframes: sf[n_sf][120*s]; result per superframe: corrected-symbol total and uncorrectable flag.
__global__ void __launch_bounds__(256) k_rs_superframes(RsArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 gtab[RS_GTAB_BYTES / 16];
    __shared__ uint8_t ws[256 * RS_WS_BYTES];
    rs_tables<256>(A.gf, alpha_to, index_of, gtab, threadIdx.x);
    __syncthreads();
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = A.n_sf * A.s;
    if (idx >= total) return;
    const int sf = idx / A.s, i = idx % A.s;
    RsIo io; io.base = A.data + (size_t)sf * A.sf_stride + i; io.pos_stride = (size_t)A.s;
    const int c = rs_decode120(io, alpha_to, index_of, gtab, ws + threadIdx.x * RS_WS_BYTES);
    if (c < 0) atomicOr(A.uncorr + sf, 1);
    else if (c > 0) atomicAdd(A.corr + sf, c);
}

// Superframes inside the MSC output of one protection class (RsMscIo)
__global__ void __launch_bounds__(256) k_rs_msc(RsMscArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t alpha_to[256], index_of[256];
    __shared__ uint4 gtab[RS_GTAB_BYTES / 16];
    __shared__ uint8_t ws[256 * RS_WS_BYTES];
    rs_tables<256>(A.gf, alpha_to, index_of, gtab, threadIdx.x);
    __syncthreads();
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int per_pair = A.n_sf_per_pair * A.s;
    if (idx >= A.n_pairs * per_pair) return;
    const int pair = idx / per_pair; const int rem = idx % per_pair;
    const int q = rem / A.s, i = rem % A.s;
    const MscPair pp = A.pairs[pair];
    const int2 rows = A.rows[pair];
    const int fc = A.first_cif[pp.ens];
    const int r0 = fc + 5 * (q + (fc < 0 ? -fc / 5 : 0));        // first logical frame of superframe q (of those that do not end in front of row 0, however far back the alignment was given)
    if (r0 < rows.x || r0 + 5 > rows.y) return;                  // a superframe that touches a row outside the batch's frames is neither decoded nor counted
    RsMscIo io;
    io.frame_bytes = A.frame_bytes; io.s = A.s; io.i = i; io.frame_stride = (size_t)A.frame_bytes;
    io.frames = A.out + ((size_t)pair * A.n_cif + r0) * A.frame_bytes;
    const int c = rs_decode120(io, alpha_to, index_of, gtab, ws + threadIdx.x * RS_WS_BYTES);
    int* cnt =A.result + 2 * ((size_t)pair * A.n_sf_per_pair + q);
    if (c < 0) atomicOr(cnt + 1, 1);
    else if (c > 0) atomicAdd(cnt, c);
}

void launch_rs_superframes(const RsArgs& a, hipStream_t s)
{
    const int total = a.n_sf * a.s;
    hipLaunchKernelGGL(k_rs_superframes, dim3((total + 255) / 256), dim3(256), 0, s, a);
}
void launch_rs_msc(const RsMscArgs& a, hipStream_t s)
{
    const int total = a.n_pairs * a.n_sf_per_pair * a.s;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_rs_msc, dim3((total + 255) / 256), dim3(256), 0, s, a);
}

} // namespace dabphy
