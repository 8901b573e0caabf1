/* include/dabphy_test.h -- test and measurement entry points of libdabphy_hip.so: timing drivers that run ONE stage alone on
 * device-resident data, and exhaustive device self-tests of two arithmetic shortcuts of the demod kernel.  tests/, tools/ and
 * bench.py's side measurements call them; a receiver needs only include/dabphy.h. */
#ifndef DABPHY_TEST_H
#define DABPHY_TEST_H

#include "dabphy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostics: time one stage on device-resident data (HIP events on the handle's stream) ------------------
 * dabphy_time_demod: tiles `n_src` host frames (layout of dabphy_demod_frames) over n_ens x n_frames frame slots in
 *   HBM and runs the demod kernel `iters` times; *ms = mean kernel time.  mix/f_hz exercise the NCO path.
 * dabphy_time_viterbi: decodes n_codewords random-content codewords of nbits `iters` times; *ms_gather / *ms_decode.
 * dabphy_time_fused_msc: re-runs the fused decode launch of the last dabphy_process batch (every class it held, the FIC included)
 *   `iters` times with nothing else on the device; *ms = mean kernel time.  DABPHY_ERR_STATE before the first such batch and after
 *   anything that replaced a buffer the launch names (dabphy_set_subchannels, a larger batch, another seam's scratch). */
int dabphy_time_demod(dabphy_handle* h, const float* frames, uint32_t n_src, uint32_t n_ens, uint32_t n_frames,
                      int32_t mix, int32_t f_hz, uint32_t iters, float* ms);
int dabphy_time_viterbi(dabphy_handle* h, uint32_t nbits, uint32_t n_codewords, uint32_t iters, float* ms_gather,
                        float* ms_decode);
int dabphy_time_fused_msc(dabphy_handle* h, uint32_t iters, float* ms);
/* dabphy_time_superframe_wide: re-runs the wide launches (k_superframe_wide, one per LDS bucket) of the last DAB+ superframe filter pass -- of
 *   dabphy_process with dabphy_set_auto_superframes, dabphy_superframes_stats or dabphy_superframes; a deferred pass that still waits runs
 *   first -- `iters` times with nothing else on the device; *ms = mean time of one repetition.  The kernel only reads the windows and the class
 *   outputs, but the pass' settle kernel has moved the windows on since: a repetition therefore leaves out, per sub-channel, the one attempt
 *   that began in frames carried into the batch (at 32 frames per batch 25 of 26 attempts, or all 25, are made again) and every sub-channel the
 *   serial walk took; each other attempt rewrites its event and superframe with the values they hold.  DABPHY_ERR_STATE before the first
 *   pass and after anything that replaced a buffer the launches name (dabphy_set_subchannels, a larger batch). */
int dabphy_time_superframe_wide(dabphy_handle* h, uint32_t iters, float* ms);
/* dabphy_get_mp2_ms: device time of the last MP2 pass (dabphy_mp2_stats / dabphy_set_auto_mp2) run with dabphy_set_profiling on; 0 if none */
int dabphy_get_mp2_ms(dabphy_handle* h, float* ms);
/* dabphy_get_chanber_ms: device time of the last channel BER pass (dabphy_set_channel_ber; both kernels) queued with dabphy_set_profiling on; 0 if none */
int dabphy_get_chanber_ms(dabphy_handle* h, float* ms);
/* EXPERIMENT of round 6, off by default (profiles/r06_viterbi_split.txt: a measured loss).  on = 1: the forward waves of the lane-per-code-word
 * Viterbi kernel publish every group's decisions (per-group scratch, agent-scope release, a flag) and walk back only when no trellis is left
 * to run -- the walks of the whole launch then overlap the forward passes of other waves instead of following each group's own.  Same bytes,
 * 6.46 against 5.74-5.87 ms for the launch alone.  on = 3 adds the 24-register walker waves (k_traceback_fused, a sixth wave per SIMD): they
 * read stale decisions across XCDs -- WRONG bytes -- and are there for the record only.  From the next batch on. */
int dabphy_test_traceback_split(dabphy_handle* h, int32_t on);
/* dabphy_time_copy: a plain device-to-device copy of `bytes` bytes (16 bytes per lane and request, grid-stride, blocks_per_cu work-groups
 *   of 256 threads per compute unit, 0 = 4), `iters` passes after three warm-up passes; *gbytes_per_s = bytes read + bytes written per
 *   second.  What the device's HBM delivers to the simplest possible kernel on this box: the measured denominator bench.py prints
 *   next to the 8 TB/s specification (tools/ubench/copy_f4.hip is the stand-alone sweep of the same kernel). */
int dabphy_time_copy(dabphy_handle* h, uint64_t bytes, uint32_t blocks_per_cu, uint32_t iters, float* gbytes_per_s);
/* dabphy_time_wideband: the channeliser's launches of the last dabphy_stream_write_wideband (k_wideband + k_wideband_carry; on a stream opened with dabphy_stream_open_resampled, k_resample + k_resample_carry) run again
 *   on its staged capture, which is still on the device: `warmup` passes, then `iters` timed one by one; ms[i] = device time of pass i.
 *   The passes rewrite the same ring samples with the same values and leave the stream's state alone.  DABPHY_ERR_STATE when no
 *   synchronous wideband write has been made since the open call. */
int dabphy_time_wideband(dabphy_handle* h, uint32_t warmup, uint32_t iters, float* ms);

/* Device self-test of the reciprocal-based 127/x the demapper uses in place of the IEEE division sequence
 * (ofdm-decoder.cpp:208 computes 127.0f / l1_norm): every float x in [2^-100, 2^100] is divided both ways on the device.
 * counts[0] = mismatches of the 4-instruction variant, counts[1] = of the 6-instruction variant, counts[2] = values tried. */
int dabphy_selftest_div127(dabphy_handle* h, uint64_t* counts);
/* Device self-test of the one-instruction product by the unit twiddle tw[0] = (1, +-0) in the first two passes of the demod kernel's
 * FFT (kiss_fft.c:21-90 multiplies by it like by any other twiddle): 2^33 operand pairs -- every exponent, zeros, denormals, infinities
 * and NaNs included -- through both forms.  counts[0] = results that differ in a bit (two NaNs count as equal), counts[1] = pairs tried. */
int dabphy_selftest_unit_twiddle(dabphy_handle* h, uint64_t* counts);
/* Device self-test of the lane exchanges of the state-parallel Viterbi kernel (k_viterbi_sp.hip: v_permlane32_swap, v_permlane16_swap,
 * bank-masked row DPP moves, quad_perm DPP reads, v_readlane) against plain shuffles: the forms the
 * GPU-less execution model of tests/hipemu stands in for.  counts[0] = mismatches, counts[1] = values checked. */
int dabphy_selftest_pair_exchange(dabphy_handle* h, uint64_t* counts);   /* (also swap16 / partner of k_viterbi_sp2.hip) */

/* Which Viterbi kernel decoded the last dabphy_process batch (dabphy_config.decode_shape = 0 leaves the choice to the library):
 * *shape = numbered like dabphy_config.decode_shape: 1 lane per code word (k_viterbi_fused), 2 state-parallel with two code words per wavefront
 * (k_viterbi_sp2 + k_traceback_sp2), 3 state-parallel with one (k_viterbi_sp), 0 nothing decoded yet; *fused_classes = protection
 * classes (not counting the FIC) that rode in that launch -- the others took the two-kernel path.  Either pointer may be NULL. */
int dabphy_last_decode_plan(dabphy_handle* h, int32_t* shape, int32_t* fused_classes);

/* Pure host query, no handle and no device: the fused decode's window schedule of a protection class (dabphy_protection_eep / _uep /
 * _fic) for the kernel's three row counts (batches of >= 64, >= 16, >= 4 CIFs).  n_windows[v] = 16-byte windows of the punctured code
 * word the schedule walks, 0 = the kernel cannot follow the profile's depuncturing map with that row count (the class then takes the
 * two-kernel path: same bytes, one more pass through HBM). */
int dabphy_test_fused_windows(const dabphy_protection* prot, int32_t n_windows[3]);

/* The TII side path (k_tii_measure + k_tii_accumulate, the launch dabphy_process makes) on host-supplied (NULL symbol, PRS) pairs as
 * OFDMProcessor hands them to TIIDecoder::pushSymbols: null [n_ens][n_frames][2656] and prs [n_ens][n_frames][2048] cf32,
 * valid [n_ens][n_frames] = FrameDesc::valid of each frame (only 1 = demodulated is analysed).  The pairs are laid out as frames in a
 * device buffer (PRS at the frame start, NULL symbol 2048 + 75 * 2552 samples behind it) with the oscillator at rest, so the kernels see
 * the samples unchanged.  The handle's own sums, tables and event buffers are used: the 5-frame sums carry from call to call and into
 * dabphy_process, dabphy_get_tii returns this call's measurements, dabphy_reset starts over.  n_ens = the handle's n_ensembles,
 * 1 <= n_frames <= max_frames; DABPHY_ERR_INVALID otherwise, and unless dabphy_set_tii(h, 1) has been called. */
int dabphy_test_tii_pairs(dabphy_handle* h, const float* null, const float* prs, const int32_t* valid, uint32_t n_ens, uint32_t n_frames);
/* Measurements per ensemble that were analysed but not added to any sum because all 32 slots of the ensemble were taken by other
 * comb/pattern pairs, since dabphy_set_tii switched the side path on for the first time or the last dabphy_reset. */
int dabphy_test_tii_dropped(dabphy_handle* h, int32_t* per_ensemble);

/* The PRS window search and the coarse corrector (sync_find_body of k_sync.hip: PhaseReference::findIndex by the handle's fft_placement,
 * OFDMProcessor::processPRS by its freqsync_method, the gate by its disable_coarse) on host-supplied cases, one per ensemble: ONE of the
 * launches dabphy_process queues -- kernel = DABPHY_TEST_SYNC_SERIAL (k_sync_find), _WIDE (k_sync_find_wide) or _CHAIN (k_sync_find_chain
 * from frame 0 on) -- with the arguments dabphy_process gives it, over a looping ring of 2 x DABPHY_TEST_SYNC_CASE samples per ensemble
 * that holds the case at position 0 and zeros behind it.
 *   iq [n_ens][DABPHY_TEST_SYNC_CASE] cf32: the search reads samples 0 .. 2047, the coarse corrector 2048 samples from the index found;
 *   coarse, fine [n_ens]: the correctors the receiver -- in lock, oscillator phase 0 -- starts with (only their sum moves the oscillator:
 *   coarse + fine = 0 leaves the samples unchanged); fic_ratio [n_ens]: the 0 .. 10 counter the gate `ratio * 10 < 50` consults.
 * n_frames = 1, or with _CHAIN up to max_frames: frame n + 1 is searched where the hand-over of frame n puts it (the ring index of a
 * frame's search is that of its predecessor + start_index + 2048 + 75 * 2552 + 2656, modulo the ring).
 * out [n_ens][n_frames], cir [n_ens][n_frames][2048] (the impulse response magnitudes; zeros where no search ran), state [n_ens]: what
 * the launch left in the receiver state (a failed serial search consumes 2048 samples and drops lock; _WIDE and _CHAIN leave it alone).
 * DABPHY_ERR_INVALID, nothing launched: n_ens != the handle's n_ensembles, a null pointer, an unknown kernel, n_frames = 0 or above
 * max_frames or (not _CHAIN) above 1.  The handle's synchroniser and decoder state are overwritten: dabphy_reset before anything else. */
#define DABPHY_TEST_SYNC_CASE 4096
enum { DABPHY_TEST_SYNC_SERIAL = 0, DABPHY_TEST_SYNC_WIDE = 1, DABPHY_TEST_SYNC_CHAIN = 2 };
typedef struct { int64_t pos; int32_t start_index, valid, coarse_ran, coarse_after, coarse_step, L1; } dabphy_test_sync_desc;   /* FrameDesc members of the same names */
typedef struct { int64_t pos; int32_t synced, lost; } dabphy_test_sync_state;
int dabphy_test_sync_find(dabphy_handle* h, int32_t kernel, const float* iq, const int32_t* coarse, const int32_t* fine, const int32_t* fic_ratio,
                          uint32_t n_ens, uint32_t n_frames, dabphy_test_sync_desc* out, float* cir, dabphy_test_sync_state* state);

/* Unit entry of the access-unit pack pass (k_au_pack, the launch behind every filter pass while dabphy_set_au_drain is on) on host-supplied
 * corrected superframes and their events, treated as ONE service: sf [n_sf][120 * s_per_sf], events [n_events] as the filter writes them
 * (sf_slot = index into sf, au_crc_ok as it stands: no CRC is checked here), format = DABPHY_AU_RAW / DABPHY_AU_LOAS.  out [out_capacity]
 * receives the service's whole reservation (out_capacity bytes, zeros behind service->bytes; the first access unit that does not fit
 * the reservation or the aus_capacity records is left out with everything behind it: n_aus and bytes count what was stored), aus [aus_capacity] its records with offsets relative to out, *service its totals.  The handle's drain is not touched. */
int dabphy_test_au_pack(dabphy_handle* h, const uint8_t* sf, const dabphy_sf_event* events, uint32_t n_events, uint32_t n_sf, uint32_t s_per_sf,
                        int32_t format, uint8_t* out, size_t out_capacity, dabphy_au_desc* aus, uint32_t aus_capacity, dabphy_au_service* service);
/* dabphy_get_au_ms: device time of the last pack pass queued with dabphy_set_profiling on; 0 if none */
int dabphy_get_au_ms(dabphy_handle* h, float* ms);

#ifdef __cplusplus
}
#endif

#endif /* DABPHY_TEST_H */
