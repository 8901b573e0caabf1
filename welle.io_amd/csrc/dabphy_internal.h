// welle.io_amd/csrc/dabphy_internal.h -- what the translation units of the C ABI share: the handle (streams, events, device buffers of one
// receiver batch), small host helpers, and the internal functions that cross files.  Not installed, not part of include/dabphy.h.
//   dabphy_api.hip          create / destroy / options / sub-channel classes, the stateless seams (demod, Viterbi, FIC, RS) and the timing drivers
//   dabphy_stream.hip       sample rings (bind / upload / write / raw formats), the wideband front end's open and write calls (dabphy_handle::Wideband), the synchroniser's chain and wide pass, reset
//   dabphy_process.hip      dabphy_process: the pipelined schedules, exact batch mode (replay), the decode of one batch as named steps
//   dabphy_fused.hip        the fused decode's host side: per-class step tables; the launch plan as named steps (fused_plan: choose_shape, admit_classes,
//                           build_work_list, lay_out_scratch, reserve_buffers, upload_changed, keep_plan), launch_plan, the one-class state-parallel launches
//   dabphy_superframes.hip  Reed-Solomon seams and the DAB+ superframe filter
//   dabphy_mp2.hip          classic DAB (MP2) services: audio kinds, the MP2 frame check and its unit entry
//   dabphy_getters.hip      everything a caller reads back after a batch, profiling, TII
//   dabphy_au.hip           the bulk access-unit drain: the pack pass behind the filter (k_au.hip), its tables and its copy to the host
//   dabphy_chanber.hip      the channel BER pass (k_chanber.hip): tables, the launch behind a batch's final decode, getters, the stateless entry
//   k_sync.hip              the synchroniser's kernels, with one header per reference function: sync_window.h (PhaseReference::findIndex:
//                           impulse response, the three window-index methods), sync_fine.h (the fine corrector's step and its interval test; host-compilable); block_reduce.h (their work-group reduction)
//   k_wideband.hip, k_resample.hip   the wideband front end's main kernels (integer, rational rate); capture_sample (dabphy_kernels.h) and k_capture_carry (k_ingest.hip) serve both
//   soft_layout.h           where a code word's soft bits lie in the soft-bit ring, for kernels and host alike (dabphy_fused.hip's step tables)
//   decode_work.h           the decoders' work-item word and the state-parallel kernels' history geometry, for kernels and host alike (through dabphy_kernels.h)
// Ownership: a device buffer (DevBuf) owns itself and is freed by its destructor; streams, events and page-locked blocks are created
// through new_stream / new_event / pinned_alloc below and nowhere else, which register them with the handle for dabphy_destroy.
#pragma once
#define DABPHY_BUILDING_LIBRARY          // (the exported symbol `dabphy_create` is the frozen round-3 entry point here, not the header's inline)
#include "../../include/dabphy.h"
#include "../../include/dabphy_test.h"
#include "dabphy_kernels.h"
#include "dabphy_host.h"
#include "osc_exact.h"
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <functional>
#include <numeric>

#define DABPHY_INTERNAL __attribute__((visibility("hidden")))

namespace dabphy {

// Environment variables are read only by builds made with -DDABPHY_EXPERIMENTS (timing / debugging builds and the GPU-less test
// build): the product library is configured through dabphy_config alone.
inline bool debug_env(const char* name)
{
#ifdef DABPHY_EXPERIMENTS
    return getenv(name) != nullptr;
#else
    (void)name; return false;
#endif
}

// A device allocation and its owner: move-only (a move leaves the source empty), freed by the destructor; dev_alloc / ensure fill it
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { hipError_t e = hipFree(p); (void)e; p = nullptr; cap = 0; } }
};

constexpr int HIST_CAP = 64;     // window searches remembered per ensemble for the sLevel replay
// superframe filter launches (dabphy_superframes.hip): a class to walk and which of its pairs (DEVICE list; nullptr: all of them)
struct SfSel { int cls; const int32_t* d_run; int n_run; };
constexpr int SP_SINGLE_MAX_GROUPS = 4096;   // groups of 64 code words a one-class state-parallel launch takes (sp_single_*: the seams, the replay's FIC)
constexpr int SF_BATCH_CLASSES = 256;                                                        // classes per bucket (a handle has at most 255)
constexpr size_t SF_BATCH_BYTES = 3 * (SF_BATCH_CLASSES * sizeof(SfArgs) + (SF_BATCH_CLASSES + 1) * sizeof(int32_t) + 12);
// DABPHY_DEBUG_TIMING=1: host-side time line of dabphy_process (microseconds since entry, averaged, printed every 8th call)
struct HostTimeline { double acc[6] = {0, 0, 0, 0, 0, 0}; long n = 0; };
} // namespace dabphy
using namespace dabphy;          // (internal header: the handle below names the kernels' argument blocks)

struct dabphy_handle {
    dabphy_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    char devname[256] = {0};
    // constant tables in HBM
    cf32 *d_tw = nullptr, *d_ref = nullptr, *d_nco = nullptr;
    int16_t* d_bin2soft = nullptr; uint32_t* d_prbs_words = nullptr; map_t* d_fic_map = nullptr;
    int32_t* d_osc_unsafe = nullptr; unsigned long long* d_osc_stats = nullptr;   // osc_exact.h: unsafe table entries; symbols mixed unchecked / checked
    Tables tab{};
    // grow-only scratch
    DevBuf iq, soft, con, prs_mag, snr, desc, in8, map, vsym, vdec, vout, ok;
    DevBuf fsym, fdec;                      // Viterbi scratch of the FIC class (it decodes beside the MSC classes on aux_stream)
    RxState* d_state = nullptr;       // [n_ensembles] synchroniser state
    DecState* d_dec = nullptr;        // [n_ensembles] decoder state
    std::vector<DevBuf> owned;        // blocks of fixed size that live as long as the handle (device_block: tables, state, flags)
    std::vector<hipStream_t> streams; std::vector<hipEvent_t> events; std::vector<void*> pinned;   // what new_stream / new_event / pinned_alloc created, each once (an alias such as fic_stream = aux_stream is not registered again): dabphy_destroy releases them

    // ---- streaming receiver (dabphy_stream_* / dabphy_process)
    // One protection class of the batch: the (ensemble, sub-channel) pairs of ALL ensembles that share a protection profile -- every
    // ensemble selects its own sub-channels (msc-handler.cpp:61-103) --, ordered by ensemble, then by position in the ensemble's list.
    struct MscClass {
        dabphy_protection prot{};
        std::vector<MscPair> pairs;          // host mirror of pair_tab
        std::vector<int32_t> subch_id, start_cu;   // per pair: Subchannel::subChId / startAddr (what identifies a running service when the lists change)
        bool cif0_pending = false;           // some pair's cif0 is still -1 on the device: the next decode resolves it (k_pair_cif0), then the mirror follows
        DevBuf map, pair_tab, tiles, out;    // depuncture map, the pair table, gather tiles, decoded bytes [pair][4F][nbits/8]
        DevBuf steps[FUSED_VARIANTS]; int n_windows[FUSED_VARIANTS] = {0, 0, 0};   // fused decode (k_viterbi_fused): per-step window-ring descriptors for each row-count build (0 windows: not decodable that way)
        DevBuf sf_state;                     // SuperframeFilter window of every pair
        size_t sf_pair0 = 0, sf_bytes0 = 0;  // this class's region of the filter's shared event / count / verdict buffers (in pairs) and of its superframe buffer (in bytes): prepare_superframes
        DevBuf sf_snap;                      // ... as it was in front of the current batch (exact batch mode)
        // classic DAB (MP2) services (dabphy_mp2.hip): the audio kind of every pair as applied, device lists of the DAB+ / MP2 pairs (only
        // when the class has an MP2 pair: otherwise the DAB+ filter walks every pair as before), the MP2 parser state and its results
        std::vector<int32_t> kind;
        DevBuf dab_run, mp2_run; int n_dab = 0, n_mp2 = 0;
        DevBuf mp2_state, mp2_snap, mp2_ev, mp2_n, mp2_err, mp2_fu;
        bool dabplus_rate() const { return (prot.nbits / 24) % 8 == 0 && prot.nbits / 8 >= 10; }
        size_t sf_stride() const { return sf_state_stride(prot.nbits / 8); }
    };
    struct PairRef { int cls = -1, pair = -1; };
    const cf32* s_iq = nullptr;       // DEVICE pointer to [B][stride] samples (caller's or s_iq_own)
    DevBuf s_iq_own;
    uint64_t s_stride = 0, s_ring = 0, s_valid = 0; int s_loop = 0;
    bool s_bounded = false;           // every sample the stream ever held came through k_ingest from u8 / s8 / s16: |re|, |im| <= 1
    // sub-channel selection: per ensemble.  `subch_e` + `classes` + `where` = what the kernels decode with; `subch_next` = what the caller
    // has asked for (dabphy_set_subchannels / _ensemble); apply_subchannels rebuilds the former from the latter (carrying the state of
    // every service that stays) before the next batch is decoded.
    std::vector<std::vector<dabphy_subchannel>> subch_e, subch_next;     // [n_ensembles]
    std::vector<std::vector<PairRef>> where;                             // [n_ensembles][position in the list] -> class, pair
    bool subch_dirty = false;
    std::vector<std::vector<int32_t>> kind_next;                         // [n_ensembles][position]: dabphy_set_audio_kinds_ensemble (reset by a new list)
    bool kinds_dirty = false;
    bool mp2_auto = false, mp2_done = false;                             // dabphy_set_auto_mp2; the MP2 pass has run for the last batch
    hipEvent_t ev_mp2[2] = {nullptr, nullptr}; bool mp2_timed = false;   // the last MP2 pass, with profiling on (dabphy_get_mp2_ms)
    DevBuf mp2_stats, mp2_chk_state, mp2_chk_ev, mp2_chk_n, mp2_chk_err, mp2_chk_fu;
    std::vector<MscClass> classes;
    DevBuf sf_batch; void* h_sf_batch = nullptr;                         // argument blocks of the filter's per-bucket launches (device, page-locked staging)
    DevBuf sf_run;                                                       // pair selections of one-sub-channel superframe filter launches
    DevBuf s_raw;                           // staging of raw-format samples (dabphy_stream_write_raw)
    DevBuf s_raw2[2]; hipStream_t copy_stream = nullptr; hipEvent_t ev_ingest[2] = {nullptr, nullptr}; int raw_sel = 0;   // dabphy_stream_write_raw_async
    uint64_t s_enqueued = 0; int commit_slot = -1;    // samples handed to the copy stream so far; slot whose event covers the committed ones
    DevBuf s_null;                          // null symbols on request (dabphy_get_null_symbols)
    // Wideband front end: one capture channelised into the ring rows, at D x 2.048 MS/s (INTEGER: dabphy_stream_open_wideband,
    // k_wideband.hip) or at 2.048 MS/s x M / L (RATIONAL: dabphy_stream_open_resampled, k_resample.hip).  The open call creates every
    // buffer -- its kind's tables, both carries, the three staging buffers at the largest write -- and a plain open or bind drops the
    // configuration (OFF; the buffers stay with the handle, grow-only like the rest).  Both kinds share the write calls and what they
    // carry: the carry (dabphy_reset clears it) and the capture index `abs`, in the order the writes are QUEUED in.  Each kind owns its
    // geometry, its tables and its last synchronous write as it was launched (`last`, with last_valid: dabphy_time_wideband runs it again).
    struct Wideband {
        enum Kind { OFF, INTEGER, RATIONAL } kind = OFF;
        int32_t format = 0;
        DevBuf carry[2]; int carry_sel = 0; uint32_t carry_len = 0;   // carry[carry_sel]: the carry_len samples in front of the next write
        uint64_t abs = 0; bool last_valid = false;               // abs: capture samples written since the open / reset, N
        struct Integer { uint32_t D = 0, n_taps = 0, e_pad = 0; DevBuf ctaps, osc, om; WidebandArgs last{}; } integer;      // (tables: WidebandArgs has their shapes)
        // exact integers beside N: frac = (N L) mod M -- the stream holds (N L - frac) / M outputs, and M - 1 - frac says where the next
        // one's newest sample lies and which phase it has; stage_samples: no write is as long as this.  (Tables: ResampleArgs)
        struct Rational { uint32_t L = 0, M = 0, J = 0; uint64_t frac = 0, stage_samples = 0; DevBuf taps, osc_hi, osc_lo; ResampleArgs last{}; } rational;
    } wb;
    // bulk MSC drain (dabphy_msc_drain_begin / _wait): the class outputs leave on a stream of their own while the next batch starts
    hipStream_t drain_stream = nullptr; hipEvent_t ev_drain_done = nullptr, ev_drain_staged = nullptr; bool drain_pending = false; DevBuf drain_stage;
    DevBuf sf_events, sf_count, sf_bytes, sf_stats, sf_gf, sf_accept; const FrameDesc* last_desc = nullptr;
    // the wide launches of the last filter pass, per bucket, as they were queued (dabphy_time_superframe_wide re-runs them alone while buf_gen is current)
    struct SfWideLaunch { SfBatch bt{}; int blocks = 0, n_cif = 0, max_s = 0; } sf_wide_last[3]; uint64_t sf_wide_gen = 0;
    static constexpr int N_DESC = 3;    // descriptor buffers: the batch being decoded + up to two synchronised ahead
    DevBuf s_desc2[N_DESC], s_cir2[N_DESC], s_soft, s_con, s_mag, s_snr, s_fib, s_ok;
    int stream_layout = 1;                          // experiments: bit 0 placeholder streams, bit 1 FIC work on the auxiliary stream, bit 3 the bulk drain on a stream of its own even when nothing is ingested asynchronously, bit 4 the SNR kernels on the main stream in front of the decoder (no gain: profiles/r06_step_variants.txt)
    hipStream_t sync_stream = nullptr;
    hipStream_t aux_stream = nullptr; hipEvent_t ev_demod_done = nullptr, ev_fic_done = nullptr, ev_chain_gate = nullptr;
    hipStream_t fic_stream = nullptr; hipEvent_t ev_aux_done = nullptr;     // FIB CRC + FIC ratio behind a fused launch; end of the auxiliary stream's work of a batch
    // fused decode (k_viterbi_fused): every class of the batch (and the FIC) in one launch.  The plan = which build, which classes, the
    // work list; rebuilt when the batch depth, the class set or a buffer address changes (dabphy_fused.hip)
    struct FusedPlan {
        bool valid = false; uint32_t F = 0; bool want_fic = false; bool fic_in = false;
        int variant = 0, n_slots = 0;
        bool use_sp = false; int sp_variant = 0; bool sp_two = false;   // ... two code words per wavefront (k_viterbi_sp2)         // the batch is small: one wavefront per code word (k_viterbi_sp) instead of 64 code words per wavefront
        std::vector<int> class_idx;                      // classes decoded by the fused launch (the others take k_msc_gather + k_viterbi)
        std::vector<FusedClass> host_cls; std::vector<uint32_t> host_work, host_dec_off;
        bool tb_split = false;                           // the launch publishes its groups' decisions for k_traceback_fused (decision scratch then always per group)
        bool dec_by_item = false;                        // decision scratch per group of 64 code words instead of per work-group (dabphy_fused.hip)
        FusedArgs args{}; uint64_t buf_gen = 0;          // the launch as it was last queued (dabphy_time_fused_msc re-runs it alone while buf_gen is current)
        bool launched = false;
    } fplan;
    DevBuf fused_cls, fused_work, fused_dec_off; uint32_t* d_fused_next = nullptr;
    // the traceback of the lane-per-code-word kernel as a pass of its own beside the forward pass (k_traceback_fused): per-item flags + cursor, its stream
    uint32_t* h_tb_gave_up = nullptr;                    // page-locked: walkers that gave up on a flag in the last launch (must be 0)
    bool tb_split = false; bool tb_no_walkers = true; DevBuf fused_done; hipStream_t tb_stream = nullptr; hipEvent_t ev_tb_fork = nullptr, ev_tb_join = nullptr;
    bool sp1_two = false;                                // the last one-class launch prepared goes to k_viterbi_sp2
    DevBuf sp1_cls, sp1_work; void* h_sp1 = nullptr;     // one-class state-parallel launches (the seams, the replay's one-frame FIC): descriptor + work list, page-locked staging
    DevBuf fic_steps[FUSED_VARIANTS]; int fic_windows[FUSED_VARIANTS] = {0, 0, 0};
    hipEvent_t ev_fused_done = nullptr;
    uint64_t buf_gen = 1;                                // bumped whenever a device buffer is reallocated or a class is rebuilt
    bool fused_msc = true;                               // MSC classes: gather inside the Viterbi kernel (DABPHY_FUSED_MSC=0: two kernels)
    uint32_t sp_max_codewords = 40960;                   // batches with at most this many code words (all classes + FIC) are decoded state-parallel: measured crossover of the whole call, profiles/r05_viterbi_sp2.txt (DABPHY_SP_MAX_CW; 0: never)
    uint32_t sp2_min_codewords = 1024;                   // ... of which those above this many take two code words per wavefront and the traceback as a pass of its own (k_viterbi_sp2 + k_traceback_sp2) (DABPHY_SP2_MIN_CW)
    uint32_t sp2_tb_resident = 512;                      // k_traceback_sp2: work-groups of four waves the device holds at once (two per compute unit: LDS); a launch of more takes three waves each (DABPHY_SP2_TB_RESIDENT)
    uint32_t sp2_tb_warm = 4;                            // k_traceback_sp2: blocks of 30 steps a stretch's walk runs in over (120 steps ~ 17 constraint lengths; DABPHY_SP2_TB_WARM)
    bool chain_early = false;                            // pipelined schedules: queue the next batch's synchroniser in front of this batch's decoder instead of behind it (DABPHY_CHAIN_EARLY)
    bool fused_fic = true;                               // the FIC rides in the same launch (DABPHY_FUSED_FIC=0: k_fic_gather + k_viterbi on the auxiliary stream)
    hipEvent_t ev_chain_beg[N_DESC]{}, ev_chain_end[N_DESC]{}; float chain_ms = 0.0f;   // duration of the sync chain that produced the current batch
    // wide synchroniser pass (all frames of a batch at once, k_sync_find_wide/_finish_wide/_validate) and its serial fall-back
    bool wide_sync = true;            // cfg.serial_sync == 0 (DABPHY_SYNC_WIDE overrides)
    DevBuf s_redo[N_DESC];            // [B] first frame slot the wide pass did not settle
    int32_t* d_any_redo = nullptr;    // [N_DESC] verdict flags in page-locked host memory: h_any_redo = the host's address, d_any_redo = the device's
    int32_t* h_any_redo = nullptr;
    bool drift_seen = false;          // the last resolved pass settled frames through the find chain (ensembles whose PRS window moves): cfg.sync_early == 0 then queues the next batch's synchroniser in FRONT of the decoder
    hipEvent_t ev_wide_done[N_DESC]{};
    hipEvent_t ev_wide_front = nullptr; bool wide_front_recorded = false;   // behind the wide pass proper of the chain queued last (cfg.sync_early == 3: the decoder's launch waits for it)
    bool wide_pending[N_DESC]{};      // the wide pass of this descriptor buffer has been queued, its verdict not yet read
    uint64_t chain_valid[N_DESC]{}; uint32_t chain_frames[N_DESC]{};   // n_valid and n_frames the chain of this buffer was queued with
    uint64_t n_wide_passes = 0, n_wide_fallbacks = 0;
    // exact batch mode (cfg.no_batch_replay == 0): state as it was in front of a batch, to replay the batch frame by frame when one of its
    // coarse-corrector decisions was taken with a stale FIC ratio and can have mattered (k_fic_ratio's verdict)
    bool exact_batch = false;
    DevBuf snap_state[N_DESC], snap_hist[N_DESC], snap_dec, snap_tii;     // (snap_hist: the synchroniser's history ring goes with its state -- an acquisition inside the first pass restarts the ring over the entries the second pass must replay)
    int32_t* d_any_eff = nullptr; int32_t* h_any_eff = nullptr;
    uint64_t n_replayed_batches = 0;
    int desc_sel = 0;                 // which of s_desc2/s_cir2 holds the batch that dabphy_process decodes next
    int ahead = 0;                    // batches whose chain has been queued but which have not been decoded yet (pipelined modes: 1 or 2 between calls)
    uint32_t presynced = 0;           // frames already synchronised ahead into s_desc2[desc_sel] (pipelined mode)
    int soft_ring = 0;
    uint32_t last_frames = 0;         // n_frames of the last dabphy_process
    HostTimeline tl; int tl_on = -1;  // (experiments builds: read through debug_env on the first call)
    float* cur_cir = nullptr;
    FrameDesc* h_desc = nullptr;      // host copy of the last batch's frame descriptors (page-locked, [B][max_frames])
    float* h_snr = nullptr;
    uint8_t *h_fib = nullptr, *h_ok = nullptr;   // ... of its FIBs [B][F][12][32] and CRC flags [B][F][12]: they cross PCIe inside the step, beside the decoder
    int32_t* h_sf_stats = nullptr;    // ... of the superframe totals when the filter rode in dabphy_process (sf.totals)
    // stage timing (HIP events on the handle's stream, recorded when profiling is on)
    enum { ST_SYNC = 0, ST_DEMOD, ST_SNR, ST_FIC, ST_MSC_GATHER, ST_MSC_VITERBI, ST_RS, ST_COUNT };
    bool profiling = false;
    hipEvent_t ev_beg[ST_COUNT]{}, ev_end[ST_COUNT]{};
    bool ev_used[ST_COUNT]{};
    DevBuf rs_first, rs_result, rs_rows;
    DevBuf s_hist;                          // [B][HIST_CAP] window searches since the last acquisition (sLevel replay in k_sync_find's acquisition head, acquire_body)
    // TII (RadioReceiverOptions::decodeTII): constants, per-batch scratch, per-ensemble sums that live across batches
    bool tii_on = false; bool tii_ran = false;
    bool track_slevel = false;        // dabphy_set_track_slevel: sLevel follows every tracked frame instead of catching up at a loss of lock
    // dabphy_set_auto_superframes: the all-sub-channel DAB+ filter as a pass of dabphy_process -- of batch k at the end of dabphy_process(k) (mode
    // 1), or in dabphy_process(k + 1) beside that batch's FFT stage (mode 2).  Only the steps sf_* below (dabphy_superframes.hip) touch this.
    //   batch k's pass, mode 2           waiting   totals      set by
    //   decoded, pass not queued         batch k   (k - 1's)   sf_batch_decoded: the end of dabphy_process(k)
    //   queued on the auxiliary stream   none      IN_FLIGHT   sf_launch_waiting: dabphy_process(k + 1), sf_flush, a second fetch
    //   waited for                       -         LANDED      sf_batch_decoded, sf_flush or a fetch (mode 1: sf_inline_pass, final with the batch)
    //   totals handed to the caller      -         EMPTY       dabphy_superframes_stats
    //   Leaving mode 2 flushes and parks the totals as LANDED (zeros if they have been fetched): the new mode does not filter the batch again.
    //   Outside mode 2 no batch waits and no pass is in flight.  dabphy_reset drops a waiting batch and mode 2's totals.
    struct SfPass {
        enum Mode { OFF, INLINE, DEFERRED } mode = OFF;              // dabphy_set_auto_superframes(0 / 1 / 2)
        const FrameDesc* desc = nullptr; uint32_t frames = 0;        // the batch that waits for its pass (desc == nullptr: none); `frames` stays the depth of the pass queued last
        enum Totals { EMPTY, IN_FLIGHT, LANDED } totals = EMPTY;     // of the pass queued last: LANDED = in h_sf_stats, not fetched yet
        bool polled = false;                                         // a fetch has been made since the last dabphy_process: the next one runs the waiting pass at once (the end of a stream)
        hipEvent_t done = nullptr;                                   // behind the deferred pass on the auxiliary stream (created with the first one)
    } sf;
    // Bulk access-unit drain (dabphy_au.hip; dabphy_set_au_drain): a pack pass behind every all-sub-channel filter pass, drained once.
    // `last` = layout and services of the pass queued last (the classes as they were THEN: a list change rebuilds them behind a flushed
    // pass), `flight` = of the pass whose drain is in flight.  Nothing here exists while the drain is off.
    struct AuDrain {
        int format = 0;                                              // DABPHY_AU_OFF / _RAW / _LOAS for the passes queued from now on
        DevBuf stage, svc, tab, src, base; std::vector<int32_t> base_host;   // staging bytes; per-service records; AU records and their sources; first service of every ensemble
        struct Layout { std::vector<dabphy_au_service> services; std::vector<uint32_t> slot; size_t bytes = 0; uint32_t n_positions = 0, au_cap = 0; int format = 0; } last, flight;   // n_positions: list positions of all ensembles (one record slot each); slot: the service's record on the device
        bool known = false;                                          // `last` describes a pass (dabphy_au_batch_size answers)
        bool packed = false, inflight = false;                       // a pass has packed and has not been drained; a drain's copies have been queued and not waited for
        hipEvent_t ev_packed = nullptr, ev_done = nullptr, ev_time[2] = {nullptr, nullptr}; bool timed = false;
        AuSvc* h_svc = nullptr; size_t h_svc_cap = 0;                // page-locked landing area of the service records
        dabphy_au_service* out_services = nullptr; bool out_aus = false;
    } au;
    // Channel BER pass (dabphy_chanber.hip, k_chanber.hip; dabphy_set_channel_ber): the decoded bits encoded again and compared with the
    // signs of the soft bits, behind the batch's final decode.  Nothing here is allocated or launched while it is off.  The counts
    // are per batch: nothing is carried, exact batch mode has nothing to put back.
    struct ChanBer {
        bool on = false, counted = false;                            // counted: counts / totals are the last batch's (dabphy_reset, a new list and switching on clear it)
        uint32_t F = 0, row_len = 0;                                 // geometry of the tables below: batch depth, 1 + the longest list
        DevBuf cls, work, first, slots, counts, totals;              // classes (the FIC last), groups of 64 code words, first record per class, first record per totals slot
        std::vector<FusedClass> host_cls; std::vector<uint32_t> host_work, host_first, host_slots;   // what the device tables hold
        hipEvent_t ev[2] = {nullptr, nullptr}; bool timed = false;   // the last pass, with profiling on (dabphy_get_chanber_ms)
    } ber;
    DevBuf ber_lin_tab, ber_lin_out;                                 // dabphy_channel_ber (the stateless entry): its class, work list and counts
    DevBuf tii_rot, tii_rank, tii_pat, tii_err, tii_likely, tii_state, tii_events, tii_nev;     // (tii_state: [B][TII_SLOTS] sums, then [B] dropped-measurement counters -- one carried block)
    uint32_t tii_max_events = 0;
};

extern "C" {       // the steps of the superframe filter's pass (dabphy_superframes.hip), one per transition of the table at dabphy_handle::SfPass
DABPHY_INTERNAL bool sf_pass_on(const dabphy_handle* h);                     // mode 1 or 2: dabphy_process reserves the filter's buffers
DABPHY_INTERNAL bool sf_windows_carried(const dabphy_handle* h);             // exact batch mode snapshots the filter's windows (for_each_carried)
DABPHY_INTERNAL int sf_flush(dabphy_handle* h);                              // audio kinds are about to change: the waiting pass runs now and is waited for
DABPHY_INTERNAL int sf_batch_begins(dabphy_handle* h, uint32_t n_frames);    // ... or the classes, or the batch depth
DABPHY_INTERNAL int sf_launch_waiting(dabphy_handle* h);                     // the previous batch's pass, on the auxiliary stream
DABPHY_INTERNAL int sf_wait_for_pass(dabphy_handle* h, hipStream_t st);      // `st` waits for a pass in flight
DABPHY_INTERNAL void sf_outputs_go(dabphy_handle* h);                        // a new decoder launch or a class rebuild: inline totals are no longer the last batch's
DABPHY_INTERNAL int sf_inline_pass(dabphy_handle* h);                        // mode 1: this batch's pass, behind its decoders
DABPHY_INTERNAL void sf_batch_decoded(dabphy_handle* h, const FrameDesc* desc, uint32_t n_frames);
DABPHY_INTERNAL int sf_stream_reset(dabphy_handle* h);                       // dabphy_reset
}

namespace dabphy {

// A handle lives on one device; HIP's current device is a property of the calling THREAD.  Every entry point makes the handle's device
// current for its duration, so that one process can own several handles on several devices (welle.io_amd/host/gpu_node_receiver.h:
// one host thread per device) and a caller's own device selection survives the call.
struct DeviceBind {
    int prev = -1; bool switched = false;
    explicit DeviceBind(const dabphy_handle* h)
    {
        if (h && hipGetDevice(&prev) == hipSuccess && prev != h->cfg.device) switched = hipSetDevice(h->cfg.device) == hipSuccess;
    }
    ~DeviceBind() { if (switched) { hipError_t e = hipSetDevice(prev); (void)e; } }
    DeviceBind(const DeviceBind&) = delete; DeviceBind& operator=(const DeviceBind&) = delete;
};

#define HIPCHK(h, call)                                                                                   \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) { (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); return DABPHY_ERR_HIP; } } while (0)

// exactly `bytes` of device memory into an EMPTY buffer (the one place the library allocates device memory)
inline int dev_alloc(dabphy_handle* h, DevBuf& b, size_t bytes)
{
    if (hipMalloc(&b.p, bytes) != hipSuccess) { h->err = "hipMalloc failed (" + std::to_string(bytes) + " bytes)"; b.p = nullptr; return DABPHY_ERR_NOMEM; }
    b.cap = bytes;
    return 0;
}

// grow-only scratch: contents are not preserved; whatever names the old address is out of date (buf_gen)
inline int ensure(dabphy_handle* h, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    b.release();
    h->buf_gen++;
    return dev_alloc(h, b, (bytes + 4095) & ~(size_t)4095);
}

// n elements that live as long as the handle (h->owned)
template <typename T> int device_block(dabphy_handle* h, T** dst, size_t n, bool zero = false)
{
    DevBuf b; int r;
    if ((r = dev_alloc(h, b, n * sizeof(T)))) return r;
    *dst = b.as<T>();
    h->owned.push_back(std::move(b));
    if (zero) HIPCHK(h, hipMemset(*dst, 0, n * sizeof(T)));
    return 0;
}

template <typename T> int upload_const(dabphy_handle* h, T** dst, const std::vector<T>& src)
{
    int r;
    if ((r = device_block(h, dst, src.size()))) return r;
    HIPCHK(h, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
// ... or a table in grow-only scratch, copied on the handle's stream: `src` stays as it is until that stream has been waited for
template <typename T> int upload_table(dabphy_handle* h, DevBuf& b, const std::vector<T>& src)
{
    if (int r = ensure(h, b, src.size() * sizeof(T))) return r;
    HIPCHK(h, hipMemcpyAsync(b.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return 0;
}
// ... or one the handle keeps a copy of (`have`), uploaded only when its contents or its buffer changed, and never replaced under an
// earlier copy that may still read it (a pageable source is not always staged before the call returns).  table_holds: the contents
// are the same; upload_kept: `have` becomes `want` and goes up -- the caller has waited for the stream if `have` was ever uploaded;
// the handle's own storage outlives the copy, which the stream orders before the launches that read the table
template <typename T> bool table_holds(const std::vector<T>& have, const std::vector<T>& want)
{
    return have.size() == want.size() && (want.empty() || !memcmp(have.data(), want.data(), want.size() * sizeof(T)));
}
template <typename T> int upload_kept(dabphy_handle* h, DevBuf& b, std::vector<T>& have, const std::vector<T>& want)
{
    have = want;
    if (!want.empty()) HIPCHK(h, hipMemcpyAsync(b.p, have.data(), want.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return 0;
}
// ... a table in a buffer of its own (the channel BER pass; the launch plan's tables move with buf_gen and share one wait: dabphy_fused.hip)
template <typename T> int upload_if_changed(dabphy_handle* h, DevBuf& b, std::vector<T>& have, const std::vector<T>& want)
{
    const void* const before = b.p;
    if (int r = ensure(h, b, std::max<size_t>(want.size(), 1) * sizeof(T))) return r;
    if (b.p == before && table_holds(have, want)) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return upload_kept(h, b, have, want);
}

// Streams (non-blocking; high_priority: the device's greatest), events (without timing unless asked) and page-locked host blocks of a
// handle: created here, registered for dabphy_destroy.  *out stays null on failure.
inline int new_stream(dabphy_handle* h, hipStream_t* out, bool high_priority = false)
{
    int lo = 0, hi = 0;
    if (high_priority && hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) hi = 0;
    hipStream_t s = nullptr;
    if ((high_priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) { h->err = "hipStreamCreate failed"; return DABPHY_ERR_HIP; }
    h->streams.push_back(s); *out = s;
    return 0;
}
inline int new_event(dabphy_handle* h, hipEvent_t* out, bool timing = false)
{
    hipEvent_t e = nullptr;
    if ((timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess) { h->err = "hipEventCreate failed"; return DABPHY_ERR_HIP; }
    h->events.push_back(e); *out = e;
    return 0;
}
template <typename T> int pinned_alloc(dabphy_handle* h, size_t bytes, T** out)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { h->err = "hipHostMalloc failed (" + std::to_string(bytes) + " bytes)"; return DABPHY_ERR_NOMEM; }
    h->pinned.push_back(p); *out = static_cast<T*>(p);
    return 0;
}

// an event of one timing run: destroyed when the driver returns, whichever way
struct ScopedEvent {
    hipEvent_t e = nullptr;
    ScopedEvent() = default; ScopedEvent(const ScopedEvent&) = delete; ScopedEvent& operator=(const ScopedEvent&) = delete;
    hipError_t create() { return hipEventCreate(&e); }
    ~ScopedEvent() { if (e) { hipError_t r = hipEventDestroy(e); (void)r; } }
    operator hipEvent_t() const { return e; }
};

// Exact batch mode's second pass is armed whenever a coarse-corrector decision can have seen a FIC ratio older than the reference's
// (ofdm-processor.cpp:397-409: the ratio of the PREVIOUS frame): batches of several frames, and ONE frame per call too when the
// synchroniser runs ahead of the decoder (pipeline_sync 1-3).  One frame per call on the serial schedule is exact by construction.
inline bool replay_armed(const dabphy_handle* h, uint32_t F) { return h->exact_batch && (F > 1 || h->cfg.pipeline_sync != 0); }

// What a batch carries over from the one before it -- THE list: exact batch mode reserves a snapshot for every entry, saves it in
// front of the first pass and puts it back in front of the second (dabphy_process.hip), dabphy_reset zeroes the live blocks
// (every = true: whatever exists, whether or not the current options would snapshot it).  fn(live block, its snapshot, bytes);
// the first non-zero return ends the walk.  Copies skip an entry whose block or snapshot does not exist (copy_carried).
// The decoders' share: decoder state, TII sums, superframe windows and MP2 parser state per class ...
template <typename Fn> int for_each_carried(dabphy_handle* h, bool every, Fn fn)
{
    int r;
    if ((r = fn((void*)h->d_dec, h->snap_dec, sizeof(DecState) * h->cfg.n_ensembles))) return r;
    if ((r = fn(h->tii_state.p, h->snap_tii, h->tii_state.cap))) return r;
    // (deferred filter: this batch's pass has not run when the batch is decoded again, nothing to put back)
    if (every || sf_windows_carried(h)) for (auto& cls : h->classes) if ((r = fn(cls.sf_state.p, cls.sf_snap, cls.sf_state.cap))) return r;
    if (every || h->mp2_auto) for (auto& cls : h->classes) if ((every || cls.n_mp2) && (r = fn(cls.mp2_state.p, cls.mp2_snap, cls.mp2_state.cap))) return r;
    return 0;
}
// ... and the synchroniser's, per descriptor buffer: its state and the history ring that state indexes.  Saved on the synchroniser's
// stream when the buffer's chain is queued (queue_chain), put back on the main stream with the rest.
template <typename Fn> int for_each_carried_sync(dabphy_handle* h, int sel, Fn fn)
{
    int r;
    if ((r = fn((void*)h->d_state, h->snap_state[sel], sizeof(RxState) * h->cfg.n_ensembles))) return r;
    return fn(h->s_hist.p, h->snap_hist[sel], (size_t)h->cfg.n_ensembles * HIST_CAP * sizeof(FrameDesc));
}
inline int copy_carried(dabphy_handle* h, void* dst, const void* src, size_t bytes, hipStream_t st)
{
    if (dst && src) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

// TII: the carried block is the slots of every ensemble followed by its dropped-measurement counters (they are saved, put back and
// reset with the sums); per-batch scratch and the argument block of launch_tii, for dabphy_process and dabphy_test_tii_pairs alike
inline size_t tii_state_bytes(uint32_t B) { return (size_t)B * TII_SLOTS * sizeof(TiiSlot) + (size_t)B * sizeof(int32_t); }
inline int32_t* tii_dropped(const dabphy_handle* h) { return reinterpret_cast<int32_t*>(h->tii_state.as<TiiSlot>() + (size_t)h->cfg.n_ensembles * TII_SLOTS); }
inline int tii_reserve(dabphy_handle* h, uint32_t B, uint32_t F)
{
    int r;
    if ((r = ensure(h, h->tii_err, (size_t)B * F * TII_MAX_LIKELY * TII_NERR * sizeof(float)))) return r;
    if ((r = ensure(h, h->tii_likely, (size_t)B * F * (1 + TII_MAX_LIKELY) * sizeof(int32_t)))) return r;
    if ((r = ensure(h, h->tii_events, (size_t)B * TII_MAX_LIKELY * h->cfg.max_frames * sizeof(TiiEvent)))) return r;
    return ensure(h, h->tii_nev, (size_t)B * sizeof(int32_t));
}
inline TiiArgs tii_args(dabphy_handle* h, const cf32* iq, size_t iq_stride, int64_t ring, const FrameDesc* desc, uint32_t B, uint32_t F)
{
    h->tii_max_events = TII_MAX_LIKELY * h->cfg.max_frames;
    TiiArgs ta{};
    ta.tab = h->tab; ta.iq = iq; ta.iq_stride = iq_stride; ta.ring = ring; ta.desc = desc; ta.n_ens = (int)B; ta.n_frames = (int)F;
    ta.rot = h->tii_rot.as<cf32>(); ta.rank = h->tii_rank.as<int32_t>(); ta.pattern = h->tii_pat.as<uint8_t>();
    ta.abs_err = h->tii_err.as<float>(); ta.likely = h->tii_likely.as<int32_t>(); ta.state = h->tii_state.as<TiiSlot>();
    ta.events = h->tii_events.as<TiiEvent>(); ta.n_events = h->tii_nev.as<int32_t>(); ta.max_events = (int)h->tii_max_events;
    ta.overflow = tii_dropped(h);
    return ta;
}

inline int sync(dabphy_handle* h)
{
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Fill a VitClass for n_cw codewords of nbits and make sure its device buffers exist.  (h->vdec is also the decision scratch of the
// fused decode: grow-only, so a buffer that is large enough for one of the two users is never shrunk under the other.)
inline int prepare_class(dabphy_handle* h, VitClass& c, int nbits, int n_cw, int dedisperse)
{
    c.nbits = nbits; c.nsteps = nbits + 6; c.n_cw = n_cw; c.n_groups = (n_cw + 63) / 64; c.dedisperse = dedisperse; c.g_begin = 0; c.g_end = c.n_groups;
    const size_t cells = (size_t)c.n_groups * c.nsteps * 64;
    int r;
    if ((r = ensure(h, h->vsym, cells * sizeof(uint32_t)))) return r;
    if ((r = ensure(h, h->vdec, cells * sizeof(uint2)))) return r;
    if ((r = ensure(h, h->vout, (size_t)c.n_groups * 64 * (nbits / 8)))) return r;
    c.sym = h->vsym.as<uint32_t>(); c.dec = h->vdec.as<uint2>(); c.out = h->vout.as<uint8_t>();
    return 0;
}
// ---- argument blocks that several translation units build, each stated once
inline VitArgs vit_args(const dabphy_handle* h, const VitClass& c) { VitArgs v{}; v.c = c; v.prbs_words = h->d_prbs_words; return v; }
// The FIC as a class of a fused or state-parallel launch: n_cw code words decoded into `out`; variant = the row-count build whose step
// table it takes, below 0: none (the one-class launches gather by the map)
inline FusedClass fic_fused_class(const dabphy_handle* h, uint8_t* out, int n_cw, int variant)
{
    FusedClass fc{}; fc.map = h->d_fic_map; fc.out = out; fc.nbits = 768; fc.nsteps = 774; fc.n_cw = n_cw; fc.n_pairs = 1; fc.kind = 1; fc.dedisperse = 1;
    if (variant >= 0) { fc.steps = h->fic_steps[variant].as<MscStep>(); fc.n_windows = h->fic_windows[variant]; }
    return fc;
}
// ... and an MSC protection class at F frames per call: every pair's 4 F code words, written to the class's output
inline FusedClass msc_fused_class(const dabphy_handle::MscClass& c, uint32_t F, int variant)
{
    FusedClass fc{}; fc.pairs = c.pair_tab.as<MscPair>(); fc.map = c.map.as<map_t>(); fc.out = c.out.as<uint8_t>(); fc.nbits = c.prot.nbits; fc.nsteps = fc.nbits + 6;
    fc.n_pairs = (int32_t)c.pairs.size(); fc.n_cw = (int32_t)(4 * F * (uint32_t)c.pairs.size()); fc.kind = 0; fc.dedisperse = 1;
    if (variant >= 0) { fc.steps = c.steps[variant].as<MscStep>(); fc.n_windows = c.n_windows[variant]; }
    return fc;
}
// the FIC of ONE class, state-parallel or through k_fic_gather + k_viterbi (dabphy_fused.hip: fic_one_prepare / fic_one_launch): what
// sp_single_ok decided, and the prepared arguments of either path
struct FicOneClass { bool sp = false; FusedArgs spa{}; FicGatherArgs g{}; VitArgs v{}; };

} // namespace dabphy

// ---- internal functions that cross translation units (C linkage like their callers, hidden from the library's export table)
extern "C" {
DABPHY_INTERNAL int reset_synchroniser(dabphy_handle* h, bool decoder_too);                       // dabphy_stream.hip
DABPHY_INTERNAL int resolve_all_chains(dabphy_handle* h);
DABPHY_INTERNAL SyncArgs sync_args(dabphy_handle* h, int sel, uint32_t F, uint64_t n_valid);
DABPHY_INTERNAL void launch_serial_chain(dabphy_handle* h, SyncArgs sa);
DABPHY_INTERNAL int queue_chain(dabphy_handle* h, int sel, uint32_t F);
DABPHY_INTERNAL int resolve_chain(dabphy_handle* h, int sel);
DABPHY_INTERNAL int prepare_superframes(dabphy_handle* h, uint32_t F);       // dabphy_superframes.hip
DABPHY_INTERNAL int apply_subchannels(dabphy_handle* h);                                          // dabphy_api.hip
DABPHY_INTERNAL int apply_audio_kinds(dabphy_handle* h);                                          // dabphy_mp2.hip
DABPHY_INTERNAL int prepare_mp2(dabphy_handle* h, uint32_t F);
DABPHY_INTERNAL int launch_mp2_pass(dabphy_handle* h, uint32_t F);
DABPHY_INTERNAL size_t mp2_stride();
DABPHY_INTERNAL int upload_pairs(dabphy_handle* h, dabphy_handle::MscClass& cls);
DABPHY_INTERNAL int fused_class_tables(dabphy_handle* h, const dabphy_protection& prot, bool fic, DevBuf (&steps)[FUSED_VARIANTS], int (&n_windows)[FUSED_VARIANTS]);   // dabphy_fused.hip
DABPHY_INTERNAL int fused_plan(dabphy_handle* h, uint32_t F, bool want_fic);
DABPHY_INTERNAL void launch_plan(const dabphy_handle* h, hipStream_t s);                                         // the plan as queued: dabphy_process's launch, dabphy_time_fused_msc
DABPHY_INTERNAL bool sp_single_ok(const dabphy_handle* h, uint64_t n_cw, int nsteps);
DABPHY_INTERNAL int sp_single_reserve(dabphy_handle* h, uint64_t n_cw, int nsteps);
DABPHY_INTERNAL int sp_single_prepare(dabphy_handle* h, const FusedClass& fc, FusedArgs& a, hipStream_t st);
DABPHY_INTERNAL int sp_variant_for(int nsteps);
DABPHY_INTERNAL int fic_one_prepare(dabphy_handle* h, FicOneClass& o, const FicGatherArgs& g, hipStream_t st);     // called once: the class's staging copies go out here
DABPHY_INTERNAL void fic_one_launch(const dabphy_handle* h, FicOneClass& o, int frame_sel, hipStream_t st);        // frame_sel as FicGatherArgs has it
// the state-parallel launch of `a`: two code words per wavefront (k_viterbi_sp2) or one (k_viterbi_sp), as sp_two_for decided when the
// decision scratch was laid out
DABPHY_INTERNAL bool sp_two_for(const dabphy_handle* h, uint64_t n_cw);
DABPHY_INTERNAL void launch_sp(const FusedArgs& a, bool two, int lds_variant, hipStream_t s);
DABPHY_INTERNAL void msc_rows_info(const dabphy_handle* h, uint32_t b, dabphy_handle::PairRef w, int32_t* first_valid, int32_t* n_rows);   // dabphy_getters.hip: rows [first_valid, n_rows) of a pair's class output are the batch's logical frames
DABPHY_INTERNAL int drain_stream_ready(dabphy_handle* h);                                         // dabphy_getters.hip: the stream both bulk drains copy on, created with the first drain
DABPHY_INTERNAL int au_pack_pass(dabphy_handle* h, const std::vector<SfSel>& sel, hipStream_t st, uint32_t F);   // dabphy_au.hip: the pack pass behind a filter pass over `sel` (nothing when the drain is off)
DABPHY_INTERNAL int au_drain_wait(dabphy_handle* h);                                             // ... host waits for an access-unit drain in flight
DABPHY_INTERNAL int drain_wait(dabphy_handle* h);                                                // dabphy_getters.hip: host waits for a bulk MSC drain in flight
DABPHY_INTERNAL int chanber_reserve(dabphy_handle* h, uint32_t F);                               // dabphy_chanber.hip: the pass's buffers and tables for this batch depth (nothing while it is off)
DABPHY_INTERNAL int chanber_pass(dabphy_handle* h, const FrameDesc* desc, uint32_t F);           // ... the pass over the batch just decoded, on the main stream
DABPHY_INTERNAL void chanber_clear(dabphy_handle* h);                                            // ... its results are no longer the last batch's
DABPHY_INTERNAL size_t soft_ens_stride(const dabphy_handle* h);                                  // bytes between the soft-bit ring slices of two ensembles
}
