// welle.io_amd/csrc/dabphy_stream.hip -- streaming receiver: sample rings, the synchroniser's launches (serial chain and wide pass), reset.
// (split from dabphy_api.hip in round 3; dabphy_internal.h has the map of the translation units)
#include "dabphy_internal.h"

using Wideband = dabphy_handle::Wideband;

extern "C" {

// =================================================================================== streaming receiver

// ---- the synchroniser's launches.  It runs on its own stream; in pipelined mode (cfg.pipeline_sync) the frames of the NEXT batch are
// synchronised while this batch is decoded on the main stream (they need only the samples and the synchroniser's own state).
// Two forms:
//   serial chain   per frame: k_sync_find (PRS window search; acquisition first for an ensemble that is not synchronised -- start of a
//                  stream, or after a failed window search in whatever slot of a batch, as the reference falls back to notSynced,
//                  ofdm-processor.cpp:347-350) then k_sync_finish (cyclic-prefix sums -> correctors -> state).  2 F dependent launches.
//   wide pass      every frame of the batch at once, each from the state a receiver IN LOCK would be in (k_sync.hip: sync_predict), then
//                  k_sync_validate accepts the frames whose assumption held and says where the serial chain has to take over.  The
//                  verdict is read by the host the next time the batch is needed (resolve_chain): in pipelined mode that is a whole
//                  decode later, so nothing waits for it.
SyncArgs sync_args(dabphy_handle* h, int sel, uint32_t F, uint64_t n_valid)
{
    SyncArgs sa{};
    sa.tab = h->tab; sa.iq = h->s_iq; sa.iq_stride = h->s_stride; sa.ring = (int64_t)h->s_ring; sa.n_valid = (int64_t)n_valid;
    sa.loop = h->s_loop; sa.state = h->d_state; sa.dec = h->d_dec; sa.desc = h->s_desc2[sel].as<FrameDesc>(); sa.n_ens = (int)h->cfg.n_ensembles; sa.n_frames = (int)F;
    sa.fft_placement = h->cfg.fft_placement; sa.disable_coarse = h->cfg.disable_coarse; sa.freqsync = h->cfg.freqsync_method;
    sa.cir = h->cfg.want_impulse_response ? h->s_cir2[sel].as<float>() : nullptr;
    sa.hist = h->s_hist.as<FrameDesc>(); sa.hist_cap = HIST_CAP;
    // |re| + |im| of a sample with |re|, |im| <= 1 after the oscillator (|o| = 1 to 1e-7) is at most sqrt(2) * sqrt(2) = 2; a little room for rounding
    sa.level_max = h->s_bounded ? 2.125f : 3.0e38f;
    return sa;
}
void launch_serial_chain(dabphy_handle* h, SyncArgs sa)
{
    for (int f = 0; f < sa.n_frames; f++) {
        sa.frame = f;
        launch_sync_find(sa, h->sync_stream);
        launch_sync_finish(sa, h->sync_stream);
        if (h->track_slevel) launch_slevel_catchup(sa, h->sync_stream);
    }
}
constexpr int N_DESC_ = dabphy_handle::N_DESC;
int queue_chain(dabphy_handle* h, int sel, uint32_t F)
{
    SyncArgs sa = sync_args(h, sel, F, h->s_valid);
    h->chain_valid[sel] = h->s_valid; h->chain_frames[sel] = F;
    // the synchroniser's share of what exact batch mode puts back (one frame per call on the serial schedule is exact by construction:
    // nothing to save).  The history ring goes with the state whose hist_head / hist_count index it: an acquisition inside the batch
    // restarts the ring at entry 0, over the window searches the second pass has to replay through the sLevel recurrence when it
    // loses lock at the same frame
    if (replay_armed(h, F) && h->snap_state[sel].p) {
        const int rc = for_each_carried_sync(h, sel, [&](void* live, DevBuf& snap, size_t bytes) { return copy_carried(h, snap.p, live, bytes, h->sync_stream); });
        if (rc) return rc;
    }
    { hipError_t e = hipEventRecord(h->ev_chain_beg[sel], h->sync_stream); (void)e; }
    // one frame per call (the real-time facade) gains nothing from the wide pass; two batches ahead its verdict would come too late
    if (h->wide_sync && F >= 2 && h->cfg.pipeline_sync != 3 && !h->track_slevel) {
        // the verdict lands in page-locked host memory straight from the last judge kernel (no copy that could queue behind a bulk
        // transfer on the DMA engines); the host clears it here: the buffer's previous pass has been resolved
        h->h_any_redo[sel] = 0; h->h_any_redo[N_DESC_ + sel] = 0;
        sa.redo_out = h->s_redo[sel].as<int32_t>(); sa.any_redo = h->d_any_redo + sel; sa.any_chain = h->d_any_redo + N_DESC_ + sel; sa.skip_wide = h->drift_seen ? 1 : 0;
        if (!h->ev_wide_front) { const int rc = new_event(h, &h->ev_wide_front); if (rc) return rc; }
        launch_sync_wide(sa, h->sync_stream, h->ev_wide_front); h->wide_front_recorded = true;
        HIPCHK(h, hipEventRecord(h->ev_wide_done[sel], h->sync_stream));
        h->wide_pending[sel] = true; h->n_wide_passes++;
    } else {
        launch_serial_chain(h, sa);
    }
    { hipError_t e = hipEventRecord(h->ev_chain_end[sel], h->sync_stream); (void)e; }
    return DABPHY_OK;
}
// reads the wide pass's verdict for descriptor buffer `sel` and queues the serial chain for what it did not settle
int resolve_chain(dabphy_handle* h, int sel)
{
    if (!h->wide_pending[sel]) return DABPHY_OK;
    HIPCHK(h, hipEventSynchronize(h->ev_wide_done[sel]));
    h->wide_pending[sel] = false;
    h->drift_seen = h->h_any_redo[N_DESC_ + sel] != 0;         // ensembles whose window moves: the next pass starts in the find chain for everybody
    if (h->h_any_redo[sel]) {
        SyncArgs sa = sync_args(h, sel, h->chain_frames[sel], h->chain_valid[sel]);
        sa.redo_from = h->s_redo[sel].as<int32_t>();
        launch_serial_chain(h, sa);
        { hipError_t e = hipEventRecord(h->ev_chain_end[sel], h->sync_stream); (void)e; }
        h->n_wide_fallbacks++;
    }
    return DABPHY_OK;
}
int resolve_all_chains(dabphy_handle* h)
{
    for (int i = 0; i < dabphy_handle::N_DESC; i++) { int r = resolve_chain(h, (h->desc_sel + i) % dabphy_handle::N_DESC); if (r) return r; }
    return DABPHY_OK;
}

// OFDMProcessor::restart (ofdm-processor.cpp:115-132) + the start of run(): correctors, phase and sync state zero, sLevel primed over
// the next T_F/2 samples (:252-255).  decoder_too (dabphy_reset: a freshly bound stream) also rewinds the stream to sample 0 and
// clears the frame counter; without it (setReceiverOptions on a running receiver) the stream goes on where the DECODED frames end:
// frames that pipelined mode had synchronised ahead are handed back, so the time de-interleavers see every CIF exactly once.
int reset_synchroniser(dabphy_handle* h, bool decoder_too)
{
    if (h->s_desc2[0].p) { int r = resolve_all_chains(h); if (r) return r; }
    if (h->sync_stream) HIPCHK(h, hipStreamSynchronize(h->sync_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t B = h->cfg.n_ensembles;
    std::vector<RxState> init(B);
    std::vector<FrameDesc> ahead;
    if (!decoder_too) {
        HIPCHK(h, hipMemcpy(init.data(), h->d_state, init.size() * sizeof(RxState), hipMemcpyDeviceToHost));
        if (h->presynced && h->ahead > 0 && h->s_desc2[h->desc_sel].p) {          // the earliest batch synchronised ahead starts where the decoded frames end
            ahead.resize((size_t)B * h->presynced);
            HIPCHK(h, hipMemcpy(ahead.data(), h->s_desc2[h->desc_sel].p, ahead.size() * sizeof(FrameDesc), hipMemcpyDeviceToHost));
        }
    }
    for (uint32_t b = 0; b < B; b++) {
        RxState& s = init[b];
        int64_t frame_no = decoder_too ? 0 : s.frame_no, pos = decoder_too ? 0 : s.pos;
        if (!ahead.empty()) { frame_no = ahead[(size_t)b * h->presynced].frame_no; pos = ahead[(size_t)b * h->presynced].pos; }
        // counters that outlive OFDMProcessor::restart (`attempts` is a member that only the end of a scan clears, ofdm-processor.h:111,
        // ofdm-processor.cpp:258-262,354) and this library's own statistics
        const RxState keep = s;
        memset(&s, 0, sizeof s);
        s.acq_phase = 0; s.acq_left = T_F / 2; s.first_lock_attempts = -1; s.frame_no = frame_no; s.pos = pos;
        if (!decoder_too) {
            s.attempts = keep.attempts; s.first_lock_attempts = keep.first_lock_attempts; s.lost = keep.lost;
            s.n_exact_sums = keep.n_exact_sums; s.n_relock_inexact = keep.n_relock_inexact; s.n_wide_frames = keep.n_wide_frames; s.n_chain_frames = keep.n_chain_frames;
        }
    }
    h->presynced = 0; h->ahead = 0;
    HIPCHK(h, hipMemcpyAsync(h->d_state, init.data(), init.size() * sizeof(RxState), hipMemcpyHostToDevice, h->stream));
    return sync(h);
}

// the wideband front end's carried state back to the start of a capture: zeros in front of sample 0
static int wideband_clear(dabphy_handle* h)
{
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));          // writes still queued there read and write the carry
    for (DevBuf& c : h->wb.carry) HIPCHK(h, hipMemsetAsync(c.p, 0, c.cap, h->stream));
    h->wb.abs = 0; h->wb.rational.frac = 0; h->wb.carry_sel = 0; h->wb.last_valid = false;
    return DABPHY_OK;
}

int dabphy_reset(dabphy_handle* h)
{
    DeviceBind dev_(h);
    if (!h) return DABPHY_ERR_INVALID;
    int r = reset_synchroniser(h, true); if (r) return r;
    if ((r = drain_wait(h)) || (r = au_drain_wait(h))) return r;       // bulk drains in flight land first; a pass not drained goes with the stream
    h->au.packed = false;
    h->desc_sel = 0; h->n_wide_passes = h->n_wide_fallbacks = 0; h->n_replayed_batches = 0;
    h->last_frames = 0; h->last_desc = nullptr;
    if ((r = sf_stream_reset(h))) return r;
    // everything the decoders carry from batch to batch starts from zero (RadioReceiver::restart_decoder; a new OFDMProcessor owns a new
    // TIIDecoder); the pair tables and their cif0 below are reset too but are no snapshot of exact batch mode, so they stand apart
    r = for_each_carried(h, true, [&](void* live, DevBuf&, size_t bytes) -> int { if (live) HIPCHK(h, hipMemsetAsync(live, 0, bytes, h->stream)); return 0; });
    if (r) return r;
    h->mp2_done = false; chanber_clear(h);
    // ... and the frame count starts over: every selected sub-channel's time de-interleaver fills again from the first CIF decoded
    for (auto& c : h->classes) { for (MscPair& p : c.pairs) p.cif0 = -1; int r2 = upload_pairs(h, c); if (r2) return r2; }
    h->tii_ran = false;
    if (h->wb.kind != Wideband::OFF && (r = wideband_clear(h))) return r;
    return sync(h);
}

int dabphy_stream_bind_device(dabphy_handle* h, const void* d_iq, uint64_t ring_samples, uint64_t stride_samples,
                              uint64_t n_valid, int32_t loop)
{
    DeviceBind dev_(h);
    if (!h || !d_iq || ring_samples < (uint64_t)T_F || stride_samples < ring_samples) return DABPHY_ERR_INVALID;
    h->s_iq = reinterpret_cast<const cf32*>(d_iq); h->s_ring = ring_samples; h->s_stride = stride_samples;
    h->s_valid = n_valid; h->s_enqueued = 0; h->commit_slot = -1; h->s_loop = loop;
    h->s_bounded = false;                                         // the caller's cf32 samples: no bound known
    h->wb.kind = Wideband::OFF; h->wb.last_valid = false;         // a stream bound or opened any other way is no wideband stream
    return dabphy_reset(h);
}

int dabphy_stream_upload(dabphy_handle* h, const float* iq, uint64_t n_samples, int32_t loop)
{
    DeviceBind dev_(h);
    if (!h || !iq || n_samples < (uint64_t)T_F) return DABPHY_ERR_INVALID;
    const size_t bytes = (size_t)h->cfg.n_ensembles * n_samples * sizeof(cf32);
    int r;
    if ((r = ensure(h, h->s_iq_own, bytes))) return r;
    HIPCHK(h, hipMemcpyAsync(h->s_iq_own.p, iq, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return dabphy_stream_bind_device(h, h->s_iq_own.p, n_samples, n_samples, n_samples, loop);
}

int dabphy_stream_open(dabphy_handle* h, uint64_t ring_samples)
{
    DeviceBind dev_(h);
    if (!h || ring_samples < 4 * (uint64_t)T_F) return DABPHY_ERR_INVALID;
    const size_t bytes = (size_t)h->cfg.n_ensembles * ring_samples * sizeof(cf32);
    int r;
    if ((r = ensure(h, h->s_iq_own, bytes))) return r;
    HIPCHK(h, hipMemsetAsync(h->s_iq_own.p, 0, bytes, h->stream));
    r = dabphy_stream_bind_device(h, h->s_iq_own.p, ring_samples, ring_samples, 0, 0);
    h->s_bounded = true;                                          // an empty ring of zeros; a cf32 write (dabphy_stream_write) lifts the bound
    return r;
}

// ---- what the write and read calls below share, each stated once.  The write calls take the handle's own ring, not a caller's buffer
static bool owns_ring(const dabphy_handle* h) { return h->s_iq_own.p && h->s_iq == h->s_iq_own.as<cf32>(); }
// a synchronous write waits for the chain that may be running ahead and, on a wideband stream, for the asynchronous writes' carry
static int writer_wait(dabphy_handle* h, bool copies_too)
{
    HIPCHK(h, hipStreamSynchronize(h->sync_stream));
    if (copies_too) HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    return DABPHY_OK;
}
// An asynchronous write takes the staging slot of the call before last -- free, and that call's host buffer with it, once its conversion
// has run -- and copies `data` there on the copy stream; behind its launches (n_appended samples) it records when the slot is free again
static int stage_acquire(dabphy_handle* h, const void* data, size_t bytes, int* slot)
{
    if (h->s_enqueued < h->s_valid) h->s_enqueued = h->s_valid;            // synchronous writes in between
    *slot = h->raw_sel; h->raw_sel ^= 1;
    HIPCHK(h, hipEventSynchronize(h->ev_ingest[*slot]));
    const int r = ensure(h, h->s_raw2[*slot], bytes);                       // (a wideband stream's open call has made it large enough)
    if (!r) HIPCHK(h, hipMemcpyAsync(h->s_raw2[*slot].p, data, bytes, hipMemcpyHostToDevice, h->copy_stream));
    return r;
}
static int stage_release(dabphy_handle* h, int slot, uint64_t n_appended) { HIPCHK(h, hipEventRecord(h->ev_ingest[slot], h->copy_stream)); h->s_enqueued += n_appended; return DABPHY_OK; }
// n ring samples from pos on: up to the ring's end, then from its start.  Piece i: at[i] into a row, n[i] long (or 0), done[i] into the span
struct RingSpan { uint64_t at[2], n[2], done[2]; };
static RingSpan ring_span(const dabphy_handle* h, uint64_t pos, uint64_t n)
{
    const uint64_t w = pos % h->s_ring, first = std::min<uint64_t>(n, h->s_ring - w);
    return RingSpan{{w, 0}, {first, n - first}, {0, first}};
}
// the plain raw writers: their checks, and the conversion of n samples per ensemble staged at `raw` to ring position `written` on
static int raw_write_check(const dabphy_handle* h, const void* data, uint64_t n_samples, int32_t format)
{
    if (!h || !data || !owns_ring(h) || n_samples == 0 || n_samples > h->s_ring || format < DABPHY_FMT_U8 || format > DABPHY_FMT_S16BE) return DABPHY_ERR_INVALID;
    return h->wb.kind != Wideband::OFF ? DABPHY_ERR_STATE : DABPHY_OK;     // a wideband stream takes the capture (dabphy_stream_write_wideband)
}
static void ingest(const dabphy_handle* h, const DevBuf& raw, uint64_t n_samples, int32_t format, uint64_t written, hipStream_t s)
{
    IngestArgs a{};
    a.raw = raw.as<uint8_t>(); a.raw_stride = n_samples * sample_bytes(format); a.iq = h->s_iq_own.as<cf32>(); a.iq_stride = h->s_stride;
    a.ring = h->s_ring; a.w = written % h->s_ring; a.n = n_samples; a.format = format;
    launch_ingest(a, (int)h->cfg.n_ensembles, s);
}

int dabphy_stream_write(dabphy_handle* h, const float* iq, uint64_t n_samples)
{
    DeviceBind dev_(h);
    if (!h || !iq || !owns_ring(h) || n_samples == 0 || n_samples > h->s_ring) return DABPHY_ERR_INVALID;
    if (h->wb.kind != Wideband::OFF) return DABPHY_ERR_STATE;     // a wideband stream takes the capture (dabphy_stream_write_wideband)
    h->s_bounded = false;                                         // cf32 from the caller: any magnitude
    if (int r = writer_wait(h, false)) return r;
    const RingSpan sp = ring_span(h, h->s_valid, n_samples);
    for (uint32_t b = 0; b < h->cfg.n_ensembles; b++) {
        cf32* dst = h->s_iq_own.as<cf32>() + (size_t)b * h->s_stride;
        const cf32* src = reinterpret_cast<const cf32*>(iq) + (size_t)b * n_samples;
        for (int i = 0; i < 2; i++) if (sp.n[i]) HIPCHK(h, hipMemcpyAsync(dst + sp.at[i], src + sp.done[i], sp.n[i] * sizeof(cf32), hipMemcpyHostToDevice, h->stream));
    }
    h->s_valid += n_samples;
    return sync(h);
}

int dabphy_stream_write_raw(dabphy_handle* h, const void* data, uint64_t n_samples, int32_t format)
{
    DeviceBind dev_(h);
    if (format == DABPHY_FMT_CF32) return dabphy_stream_write(h, reinterpret_cast<const float*>(data), n_samples);
    int r;
    if ((r = raw_write_check(h, data, n_samples, format))) return r;
    const size_t bytes = (size_t)h->cfg.n_ensembles * n_samples * sample_bytes(format);
    if ((r = ensure(h, h->s_raw, bytes)) || (r = writer_wait(h, false))) return r;
    HIPCHK(h, hipMemcpyAsync(h->s_raw.p, data, bytes, hipMemcpyHostToDevice, h->stream));
    ingest(h, h->s_raw, n_samples, format, h->s_valid, h->stream);
    h->s_valid += n_samples;
    return sync(h);
}

int dabphy_stream_read(dabphy_handle* h, uint32_t ensemble, uint64_t pos, uint64_t n_samples, float* out)
{
    DeviceBind dev_(h);
    if (!h || !out || !h->s_iq || ensemble >= h->cfg.n_ensembles || n_samples == 0 || n_samples > h->s_ring) return DABPHY_ERR_INVALID;
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    const cf32* src = h->s_iq + (size_t)ensemble * h->s_stride;
    const RingSpan sp = ring_span(h, pos, n_samples);
    for (int i = 0; i < 2; i++) if (sp.n[i]) HIPCHK(h, hipMemcpyAsync(out + 2 * sp.done[i], src + sp.at[i], sp.n[i] * sizeof(cf32), hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

int dabphy_stream_write_raw_async(dabphy_handle* h, const void* data, uint64_t n_samples, int32_t format)
{
    DeviceBind dev_(h);
    int r, slot;
    if ((r = raw_write_check(h, data, n_samples, format)) ||
        (r = stage_acquire(h, data, (size_t)h->cfg.n_ensembles * n_samples * sample_bytes(format), &slot))) return r;
    ingest(h, h->s_raw2[slot], n_samples, format, h->s_enqueued, h->copy_stream);
    return stage_release(h, slot, n_samples);
}

// ---- wideband front end: one capture, channelised into every ensemble's ring row (k_wideband.hip; at a rational rate k_resample.hip)
// What the two open calls do once their own limits and geometry have passed (a refused open leaves the stream there was): the ring
// and the reset, which drop an earlier configuration (the kind is OFF until all is in place); both carries and the three staging buffers
// at stage_samples, more than the largest write; the kind's geometry and tables (upload_tables); the carried state at a capture's start
static int wideband_open(dabphy_handle* h, uint64_t ring_samples, Wideband::Kind kind, int32_t format, uint32_t carry_len, uint64_t stage_samples, const std::function<int()>& upload_tables)
{
    int r;
    if ((r = dabphy_stream_open(h, ring_samples))) return r;
    const size_t carry_bytes = (size_t)std::max<uint32_t>(carry_len, 1) * sizeof(cf32), stage = (size_t)stage_samples * sample_bytes(format);
    if ((r = ensure(h, h->wb.carry[0], carry_bytes)) || (r = ensure(h, h->wb.carry[1], carry_bytes)) ||
        (r = ensure(h, h->s_raw, stage)) || (r = ensure(h, h->s_raw2[0], stage)) || (r = ensure(h, h->s_raw2[1], stage)) || (r = upload_tables())) return r;
    h->wb.kind = kind; h->wb.format = format; h->wb.carry_len = carry_len;
    h->s_bounded = false;                                         // a FIR's output: no bound known (the sLevel bracket of sync_args relies on one)
    return (r = wideband_clear(h)) ? r : sync(h);                 // (the caller's host tables go out of scope)
}

int dabphy_stream_open_wideband(dabphy_handle* h, uint64_t ring_samples, const dabphy_wideband_config* cfg)
{
    DeviceBind dev_(h);
    if (!h || !cfg || cfg->struct_size != sizeof(dabphy_wideband_config) || !cfg->taps || !cfg->offset_16khz) return DABPHY_ERR_INVALID;
    const uint32_t D = cfg->decimation, n_taps = cfg->n_taps, B = h->cfg.n_ensembles;
    if (D < 1 || D > (uint32_t)WB_MAX_D || n_taps < 1 || n_taps > (uint32_t)WB_MAX_TAPS || cfg->format < DABPHY_FMT_CF32 || cfg->format > DABPHY_FMT_S16BE) return DABPHY_ERR_INVALID;
    for (uint32_t e = 0; e < B; e++) if (cfg->offset_16khz[e] > 64 * (int32_t)D || cfg->offset_16khz[e] < -64 * (int32_t)D) return DABPHY_ERR_INVALID;
    WidebandArgs geo{}; geo.D = D; geo.n_taps = n_taps;
    if (!wideband_geometry(geo)) return DABPHY_ERR_INVALID;
    // tables, in double precision, rounded once: the oscillator over its period, every ensemble's offset mod P, its taps turned by +theta k
    const uint32_t P = 128 * D, e_pad = (B + WB_ENS_STEP - 1) / WB_ENS_STEP * WB_ENS_STEP;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<cf32> osc(P), ctaps((size_t)wideband_reach(n_taps) * e_pad, cf32{0.0f, 0.0f});      // (rows of zeros behind the filter: the kernel fetches whole steps, one ahead)
    std::vector<uint32_t> om(B);
    for (uint32_t p = 0; p < P; p++) { const double a = -two_pi * (double)p / (double)P; osc[p].re = (float)cos(a); osc[p].im = (float)sin(a); }
    for (uint32_t e = 0; e < B; e++) {
        om[e] = (uint32_t)(((int64_t)cfg->offset_16khz[e] % (int64_t)P + (int64_t)P) % (int64_t)P);
        for (uint32_t k = 0; k < n_taps; k++) {
            const double a = two_pi * (double)(((uint64_t)om[e] * k) % P) / (double)P, t = (double)cfg->taps[k];
            ctaps[(size_t)k * e_pad + e].re = (float)(t * cos(a)); ctaps[(size_t)k * e_pad + e].im = (float)(t * sin(a));
        }
    }
    // the largest write fills the ring: ring x D samples
    return wideband_open(h, ring_samples, Wideband::INTEGER, cfg->format, n_taps - 1, ring_samples * D, [&]() -> int {
        Wideband::Integer& w = h->wb.integer; w.D = D; w.n_taps = n_taps; w.e_pad = e_pad;
        int r; return (r = upload_table(h, w.osc, osc)) || (r = upload_table(h, w.ctaps, ctaps)) ? r : upload_table(h, w.om, om);
    });
}

// ---- ... at 2.048 MS/s x M / L
int dabphy_stream_open_resampled(dabphy_handle* h, uint64_t ring_samples, const dabphy_resampler_config* cfg)
{
    DeviceBind dev_(h);
    if (!h || !cfg || cfg->struct_size != sizeof(dabphy_resampler_config) || !cfg->taps || !cfg->offset_16khz) return DABPHY_ERR_INVALID;
    const uint32_t L = cfg->interpolation, M = cfg->decimation, n_taps = cfg->n_taps, B = h->cfg.n_ensembles;
    if (L < 1 || L > (uint32_t)RS_MAX_L || M < 1 || M > (uint32_t)RS_MAX_M || M < L || M > (uint32_t)RS_MAX_RATIO * L || std::gcd(L, M) != 1 ||
        n_taps < 1 || n_taps > (uint32_t)RS_MAX_TAPS_PER_PHASE * L || cfg->format < DABPHY_FMT_CF32 || cfg->format > DABPHY_FMT_S16BE) return DABPHY_ERR_INVALID;
    for (uint32_t e = 0; e < B; e++) if (std::abs((int64_t)cfg->offset_16khz[e]) * (int64_t)L > 64 * (int64_t)M) return DABPHY_ERR_INVALID;
    // taps per phase as the kernel adds them: whole fetch steps (zero taps behind a phase's last)
    const uint32_t J = ((n_taps + L - 1) / L + RS_TAP_STEP - 1) / RS_TAP_STEP * RS_TAP_STEP;
    ResampleArgs geo{}; geo.L = L; geo.M = M; geo.J = J;
    if (!resample_geometry(geo)) return DABPHY_ERR_INVALID;
    // tables, in double precision, rounded once: every ensemble's oscillator at the multiples of RS_OSC_LO and at the RS_OSC_LO indices below
    // one, each from the exact phase (offset L i) mod P -- the product exceeds 2^32; the prototype
    const uint32_t P = 128 * M;
    const double two_pi = 6.283185307179586476925286766559;
    const uint32_t n_hi = (P + RS_OSC_LO - 1) / RS_OSC_LO;
    std::vector<cf32> osc_hi((size_t)B * n_hi), osc_lo((size_t)B * RS_OSC_LO);
    std::vector<float> taps((size_t)(J + RS_TAP_STEP) * L, 0.0f);     // [j][r] = h[r + j L]: the prototype as it is, zeros up to J rows and one more fetch step
    const auto turn = [&](uint64_t step, uint64_t i) { const double a = -two_pi * (double)((step * i) % P) / (double)P; return cf32{(float)cos(a), (float)sin(a)}; };
    for (uint32_t e = 0; e < B; e++) {
        const uint64_t step = (uint64_t)((((int64_t)cfg->offset_16khz[e] * (int64_t)L) % (int64_t)P + (int64_t)P) % (int64_t)P);
        for (uint32_t hi = 0; hi < n_hi; hi++) osc_hi[(size_t)e * n_hi + hi] = turn(step, (uint64_t)hi * RS_OSC_LO);
        for (uint32_t lo = 0; lo < (uint32_t)RS_OSC_LO; lo++) osc_lo[(size_t)e * RS_OSC_LO + lo] = turn(step, lo);
    }
    for (uint32_t k = 0; k < n_taps; k++) taps[k] = cfg->taps[k];
    // the largest write the ring takes: fewer than (ring + 1) M / L samples
    const uint64_t stage_samples = (ring_samples + 1) * M / L + 1;
    return wideband_open(h, ring_samples, Wideband::RATIONAL, cfg->format, J - 1, stage_samples, [&]() -> int {
        Wideband::Rational& w = h->wb.rational; w.L = L; w.M = M; w.J = J; w.stage_samples = stage_samples;
        int r; return (r = upload_table(h, w.osc_hi, osc_hi)) || (r = upload_table(h, w.taps, taps)) ? r : upload_table(h, w.osc_lo, osc_lo);
    });
}

// outputs a write of n capture samples appends to a resampled stream: floor((N + n) L / M) - floor(N L / M), from frac = (N L) mod M
static uint64_t resample_outputs(const dabphy_handle* h, uint64_t n) { return (h->wb.rational.frac + n * h->wb.rational.L) / h->wb.rational.M; }
// Source and destination of one write's launch, for either kind: n capture samples staged at `raw` behind the carry, outputs from ring
// position `written` on.  The write is then counted: the capture index moves on and the carries swap (when there is one to write)
static void wideband_ends(dabphy_handle* h, const void* raw, uint64_t n, uint64_t written, CaptureSrc& src, cf32*& carry_out, RingDst& dst)
{
    Wideband& wb = h->wb;
    src = CaptureSrc{reinterpret_cast<const uint8_t*>(raw), wb.format, n, wb.carry[wb.carry_sel].as<cf32>(), wb.carry_len};
    carry_out = wb.carry[wb.carry_sel ^ 1].as<cf32>();
    dst = RingDst{h->s_iq_own.as<cf32>(), h->s_stride, h->s_ring, written % h->s_ring};
    wb.abs += n; if (wb.carry_len) wb.carry_sel ^= 1;
}
static ResampleArgs resample_args(dabphy_handle* h, const void* raw, uint64_t n, uint64_t written)
{
    Wideband::Rational& w = h->wb.rational;
    ResampleArgs a{};
    a.L = w.L; a.M = w.M; a.J = w.J; resample_geometry(a); a.n_out = resample_outputs(h, n);
    a.taps = w.taps.as<float>(); a.osc_hi = w.osc_hi.as<cf32>(); a.osc_lo = w.osc_lo.as<cf32>();
    a.P = 128 * w.M; a.n_hi = (a.P + RS_OSC_LO - 1) / RS_OSC_LO; a.n_ens = h->cfg.n_ensembles; a.abs_mod = (uint32_t)(h->wb.abs % a.P);
    // the next output m = (N L - frac) / M: m M + M - 1 = N L + (M - 1 - frac), so its newest sample is N + (M - 1 - frac) div L
    const uint64_t ahead = w.M - 1 - w.frac;
    a.a0 = (uint32_t)(ahead / w.L); a.r0 = (uint32_t)(ahead % w.L);
    w.frac = (w.frac + n * w.L) % w.M;
    wideband_ends(h, raw, n, written, a.src, a.carry_out, a.dst);
    return a;
}
static WidebandArgs wideband_args(dabphy_handle* h, const void* raw, uint64_t n, uint64_t written)
{
    const Wideband::Integer& w = h->wb.integer;
    WidebandArgs a{};
    a.D = w.D; a.n_taps = w.n_taps; wideband_geometry(a); a.n_out = n / w.D;
    a.ctaps = w.ctaps.as<cf32>(); a.osc = w.osc.as<cf32>(); a.om = w.om.as<uint32_t>();
    a.P = 128 * w.D; a.n_ens = h->cfg.n_ensembles; a.e_pad = w.e_pad; a.abs_mod = (uint32_t)(h->wb.abs % a.P);
    wideband_ends(h, raw, n, written, a.src, a.carry_out, a.dst);
    return a;
}
static int wideband_write_check(const dabphy_handle* h, const void* data, uint64_t n)
{
    if (!h || !data) return DABPHY_ERR_INVALID;
    if (h->wb.kind == Wideband::OFF || !owns_ring(h)) return DABPHY_ERR_STATE;
    if (h->wb.kind == Wideband::RATIONAL) return n == 0 || n >= h->wb.rational.stage_samples || resample_outputs(h, n) > h->s_ring ? DABPHY_ERR_INVALID : DABPHY_OK;
    return n == 0 || n % h->wb.integer.D || n / h->wb.integer.D > h->s_ring ? DABPHY_ERR_INVALID : DABPHY_OK;
}
// queues one write's launches on `s` and says how many outputs they append; `keep`: dabphy_time_wideband runs these launches again
static uint64_t wideband_launch(dabphy_handle* h, const void* raw, uint64_t n, uint64_t written, hipStream_t s, bool keep)
{
    if (keep) h->wb.last_valid = true;
    if (h->wb.kind == Wideband::RATIONAL) {
        const ResampleArgs a = resample_args(h, raw, n, written);
        if (keep) h->wb.rational.last = a;
        launch_resample(a, s);
        return a.n_out;
    }
    const WidebandArgs a = wideband_args(h, raw, n, written);
    if (keep) h->wb.integer.last = a;
    launch_wideband(a, s);
    return a.n_out;
}
static void wideband_launch_last(dabphy_handle* h) { if (h->wb.kind == Wideband::RATIONAL) launch_resample(h->wb.rational.last, h->stream); else launch_wideband(h->wb.integer.last, h->stream); }

int dabphy_stream_write_wideband(dabphy_handle* h, const void* data, uint64_t n_capture_samples)
{
    DeviceBind dev_(h);
    int r;
    if ((r = wideband_write_check(h, data, n_capture_samples))) return r;
    if (h->s_enqueued > h->s_valid) return DABPHY_ERR_STATE;     // asynchronous writes not committed: this one would not continue them
    if ((r = writer_wait(h, true))) return r;
    HIPCHK(h, hipMemcpyAsync(h->s_raw.p, data, (size_t)n_capture_samples * sample_bytes(h->wb.format), hipMemcpyHostToDevice, h->stream));
    h->s_valid += wideband_launch(h, h->s_raw.p, n_capture_samples, h->s_valid, h->stream, true);
    return sync(h);
}

int dabphy_stream_write_wideband_async(dabphy_handle* h, const void* data, uint64_t n_capture_samples)
{
    DeviceBind dev_(h);
    int r, slot;
    if ((r = wideband_write_check(h, data, n_capture_samples)) || (r = stage_acquire(h, data, (size_t)n_capture_samples * sample_bytes(h->wb.format), &slot))) return r;
    return stage_release(h, slot, wideband_launch(h, h->s_raw2[slot].p, n_capture_samples, h->s_enqueued, h->copy_stream, false));
}

int dabphy_time_wideband(dabphy_handle* h, uint32_t warmup, uint32_t iters, float* ms)
{
    DeviceBind dev_(h);
    if (!h || !ms || iters == 0) return DABPHY_ERR_INVALID;
    if (h->wb.kind == Wideband::OFF || !h->wb.last_valid) return DABPHY_ERR_STATE;
    if (int r = writer_wait(h, true)) return r;
    ScopedEvent e0, e1;
    HIPCHK(h, e0.create()); HIPCHK(h, e1.create());
    for (uint32_t i = 0; i < warmup; i++) wideband_launch_last(h);
    for (uint32_t i = 0; i < iters; i++) {
        HIPCHK(h, hipEventRecord(e0, h->stream));
        wideband_launch_last(h);
        HIPCHK(h, hipEventRecord(e1, h->stream));
        HIPCHK(h, hipEventSynchronize(e1));
        HIPCHK(h, hipEventElapsedTime(&ms[i], e0, e1));
    }
    return sync(h);
}

int dabphy_stream_commit(dabphy_handle* h)
{
    DeviceBind dev_(h);
    if (!h) return DABPHY_ERR_INVALID;
    if (h->s_enqueued > h->s_valid) { h->s_valid = h->s_enqueued; h->commit_slot = h->raw_sel ^ 1; }
    return DABPHY_OK;
}

int dabphy_host_alloc(size_t bytes, void** out)
{
    if (!out || !bytes) return DABPHY_ERR_INVALID;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DABPHY_OK : DABPHY_ERR_NOMEM;
}

void dabphy_host_free(void* p) { if (p) { hipError_t e = hipHostFree(p); (void)e; } }

uint64_t dabphy_stream_consumed(dabphy_handle* h)
{
    DeviceBind dev_(h);
    if (!h) return 0;
    std::vector<RxState> st(h->cfg.n_ensembles);
    if (hipStreamSynchronize(h->sync_stream) != hipSuccess) return 0;
    if (hipMemcpy(st.data(), h->d_state, st.size() * sizeof(RxState), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    uint64_t m = ~0ull;
    for (auto& s : st) m = std::min<uint64_t>(m, (uint64_t)s.pos);
    return m;
}

} // extern "C"
