// welle.io_amd/csrc/dabphy_process.hip -- dabphy_process: one batch through the synchroniser, the demod kernel, the FIC and MSC decoders; pipelined schedules; exact batch mode.
// (split from dabphy_api.hip in round 3; dabphy_internal.h has the map of the translation units)
// dabphy_process at the end of the file is the schedule; every step it names is a function above it, in the order in which a batch meets them.
#include "dabphy_internal.h"

static inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One call's batch: what every step below needs beside the handle
struct Batch {
    uint32_t B = 0, F = 0;
    int cur = 0, depth = 0;                  // descriptor buffer of the batch being decoded; batches the synchroniser runs ahead of the decoder
    int ring_frames = 0; size_t ens_stride = 0;
    FrameDesc* d_desc = nullptr;
    DemodArgs da{};                          // the demod launch of the whole batch
    VitClass fic{};                          // the FIC of the whole batch as a class of its own (4 B F code words)
    double t0 = 0.0, t[6] = {0, 0, 0, 0, 0, 0};      // host time line (handle: tl_on)
};

static void tick(const dabphy_handle* h, Batch& b, int i) { if (h->tl_on) b.t[i] = now_us() - b.t0; }
static void mark(dabphy_handle* h, int stage, bool end, hipStream_t st = nullptr)
{
    if (!h->profiling) return;
    hipError_t e = hipEventRecord(end ? h->ev_end[stage] : h->ev_beg[stage], st ? st : h->stream); (void)e;
    h->ev_used[stage] = true;
}

// ---- the repeated argument blocks, each built in one place
// the FIC as a Viterbi class of n_cw code words: its own scratch, decoded into the head of the FIB buffer
static VitClass fic_class(const dabphy_handle* h, int n_cw)
{
    VitClass c{};
    c.nbits = 768; c.nsteps = 774; c.n_cw = n_cw; c.n_groups = (n_cw + 63) / 64; c.dedisperse = 1; c.g_begin = 0; c.g_end = c.n_groups;
    c.sym = h->fsym.as<uint32_t>(); c.dec = h->fdec.as<uint2>(); c.out = h->s_fib.as<uint8_t>();
    return c;
}
static FicGatherArgs fic_gather_args(const dabphy_handle* h, const Batch& b, const VitClass& c)
{
    FicGatherArgs g{}; g.soft = b.da.soft; g.soft_ring = b.ring_frames; g.frame_stride = SOFT_PER_FRAME; g.soft_ens_stride = b.ens_stride; g.desc = b.d_desc;
    g.n_ens = (int)b.B; g.n_frames = (int)b.F; g.map = h->d_fic_map; g.c = c;
    return g;
}
static CrcArgs crc_args(const dabphy_handle* h, const Batch& b)
{
    CrcArgs k{}; k.fib = b.fic.out; k.ok = h->s_ok.as<uint8_t>(); k.state = h->d_dec; k.desc = b.d_desc; k.n_ens = (int)b.B; k.n_frames = (int)b.F; k.disable_coarse = h->cfg.disable_coarse;
    return k;
}
static DemodArgs demod_args(const dabphy_handle* h, const Batch& b)
{
    DemodArgs da{};
    da.tab = h->tab; da.iq = h->s_iq; da.iq_stride = h->s_stride; da.ring = (int64_t)h->s_ring;
    da.desc = b.d_desc; da.n_frames = (int)b.F; da.chunk_len = h->cfg.demod_chunk; da.mix = 1;
    da.soft = h->s_soft.as<int8_t>(); da.soft_ring = b.ring_frames; da.soft_ens_stride = b.ens_stride;
    da.con = h->cfg.want_constellation ? h->s_con.as<cf32>() : nullptr; da.prs_mag = h->s_mag.as<float>();
    da.osc_stats = h->d_osc_stats;
    return da;
}
// class ci rides in the fused launch (the others take k_msc_gather + k_viterbi)
static bool in_fused_launch(const dabphy_handle* h, size_t ci)
{
    return std::find(h->fplan.class_idx.begin(), h->fplan.class_idx.end(), (int)ci) != h->fplan.class_idx.end();
}

// ---- every allocation this call may need happens here, before any kernel is queued or any pipeline state advances: a failed
// hipMalloc leaves the handle as it was
static int reserve_batch(dabphy_handle* h, const Batch& b)
{
    const uint32_t B = b.B, F = b.F;
    int r;
    for (int k = 0; k < dabphy_handle::N_DESC; k++) {
        if ((r = ensure(h, h->s_desc2[k], (size_t)B * h->cfg.max_frames * sizeof(FrameDesc)))) return r;
        if ((r = ensure(h, h->s_redo[k], (size_t)B * sizeof(int32_t)))) return r;
        if (h->cfg.want_impulse_response && (r = ensure(h, h->s_cir2[k], (size_t)B * h->cfg.max_frames * T_U * sizeof(float)))) return r;
    }
    {   // [B][ring_frames frame slots + one frame of zeros]: the zeros are what the fused decode loads for CIFs that do not exist yet
        // (nothing ever writes them; one sub-channel's worth -- 864 CU x 64 bits -- is the most a row needs)
        const size_t ring_bytes = (size_t)B * b.ens_stride;
        if (h->s_soft.cap < ring_bytes) {
            if ((r = ensure(h, h->s_soft, ring_bytes))) return r;
            for (uint32_t e = 0; e < B; e++) HIPCHK(h, hipMemsetAsync(h->s_soft.as<int8_t>() + (size_t)e * b.ens_stride + (size_t)b.ring_frames * SOFT_PER_FRAME, 0, SOFT_PER_FRAME, h->stream));
        }
    }
    const VitClass fic = fic_class(h, (int)(B * F * 4));
    if ((r = ensure(h, h->s_hist, (size_t)B * HIST_CAP * sizeof(FrameDesc)))) return r;
    if ((r = ensure(h, h->s_mag, (size_t)B * F * T_U * sizeof(float)))) return r;
    if ((r = ensure(h, h->s_snr, (size_t)B * F * sizeof(float)))) return r;
    if ((r = ensure(h, h->s_fib, std::max((size_t)B * F * 384, (size_t)fic.n_groups * 64 * 96)))) return r;      // the class output holds whole groups of 64 codewords
    if ((r = ensure(h, h->s_ok, (size_t)B * F * 12))) return r;
    if (h->cfg.want_constellation && (r = ensure(h, h->s_con, (size_t)B * F * 1200 * sizeof(cf32)))) return r;
    if (h->tii_on && (r = tii_reserve(h, B, F))) return r;
    for (auto& cls : h->classes) {
        const size_t n_groups = ((size_t)4 * F * cls.pairs.size() + 63) / 64;
        if ((r = ensure(h, cls.out, n_groups * 64 * (cls.prot.nbits / 8)))) return r;
    }
    if (sf_pass_on(h) && (r = prepare_superframes(h, F))) return r;
    if (h->mp2_auto && (r = prepare_mp2(h, F))) return r;
    // (the replay of exact batch mode decodes one frame's FIC at a time, state-parallel when 4 B code words are few: its buffers now)
    if (replay_armed(h, F) && sp_single_ok(h, (uint64_t)B * 4, fic.nsteps) && (r = sp_single_reserve(h, (uint64_t)B * 4, fic.nsteps))) return r;
    // the fused decode of this batch depth: which classes (and whether the FIC) ride in the one launch; its decision scratch
    if ((r = fused_plan(h, F, true))) return r;
    // what is left for the two-kernel path: Viterbi scratch of the largest such class; the FIC's own (the replay of exact batch
    // mode decodes one frame's 4 B code words at a time through it even when the batch's FIC is fused)
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        VitClass c{};
        if (!in_fused_launch(h, ci) && (r = prepare_class(h, c, h->classes[ci].prot.nbits, (int)(4 * F * h->classes[ci].pairs.size()), 1))) return r;
    }
    const size_t fic_groups = h->fplan.fic_in ? ((size_t)B * 4 + 63) / 64 : (size_t)fic.n_groups;
    if (!h->fplan.fic_in || h->exact_batch) {
        if ((r = ensure(h, h->fsym, fic_groups * fic.nsteps * 64 * sizeof(uint32_t)))) return r;
        if ((r = ensure(h, h->fdec, fic_groups * fic.nsteps * 64 * sizeof(uint2)))) return r;
    }
    if (sf_pass_on(h) && (r = ensure(h, h->sf_stats, sizeof(int32_t) * 4 * B))) return r;
    if (h->exact_batch) {       // a snapshot for everything a batch carries (dabphy_internal.h: for_each_carried)
        const auto reserve = [&](void*, DevBuf& snap, size_t bytes) { return ensure(h, snap, bytes); };
        for (int k = 0; k < dabphy_handle::N_DESC; k++) if ((r = for_each_carried_sync(h, k, reserve))) return r;
        if ((r = for_each_carried(h, false, reserve))) return r;
    }
    if ((r = chanber_reserve(h, F))) return r;                // (dabphy_set_channel_ber: tables over the class outputs as they now lie)
    // (an ensure() above may have moved a buffer the plan names: then it is stale -- plan again, nothing moves the second time)
    if (h->fplan.buf_gen != h->buf_gen && (r = fused_plan(h, F, true))) return r;
    // split traceback: the page-locked word the walkers' give-up count comes back in
    if (h->fplan.args.n_work > 0 && h->fplan.args.done && !h->h_tb_gave_up && (r = pinned_alloc(h, sizeof(uint32_t), &h->h_tb_gave_up))) return r;
    return 0;
}

// asynchronous ingest: everything committed must have landed before this call's kernels read the ring (the copy stream is
// in order, the event of the last committed write covers the older ones); uncommitted writes keep flowing meanwhile
static int wait_for_ingest(dabphy_handle* h)
{
    if (h->commit_slot < 0) return 0;
    HIPCHK(h, hipStreamWaitEvent(h->sync_stream, h->ev_ingest[h->commit_slot], 0));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_ingest[h->commit_slot], 0));
    h->commit_slot = -1;
    return 0;
}

// Exact batch mode: what the decoders carry from batch to batch, as it is in front of this one (the synchroniser's share was saved
// when this batch's chain was queued: queue_chain) ...
static int save_carried(dabphy_handle* h)
{
    int r = for_each_carried(h, false, [&](void* live, DevBuf& snap, size_t bytes) { return copy_carried(h, snap.p, live, bytes, h->stream); });
    if (r) return r;
    HIPCHK(h, hipMemsetAsync(h->d_any_eff, 0, sizeof(int32_t), h->stream));
    return 0;
}
// ... and put back: synchroniser state (as saved when its chain was queued), decoder state, TII sums, superframe windows, MP2 parsers
static int restore_carried(dabphy_handle* h, int cur)
{
    const auto put_back = [&](void* live, DevBuf& snap, size_t bytes) { return copy_carried(h, live, snap.p, bytes, h->stream); };
    int r;
    if ((r = for_each_carried_sync(h, cur, put_back))) return r;
    if ((r = for_each_carried(h, false, put_back))) return r;
    HIPCHK(h, hipMemsetAsync(h->d_any_eff, 0, sizeof(int32_t), h->stream));
    return 0;
}

// Exact batch mode, second pass: the batch again, frame by frame, with the reference's own feedback -- the window search of
// frame f consults the FIC ratio as it stands after frame f - 1 (ofdm-processor.cpp:397), which takes that frame's FIC: chain
// step, the first chunk(s) of the frame's symbols (PRS + the three FIC symbols), FIC decode of the class, ratio of frame f.  Everything else
// of the batch follows in decode_batch as in the first pass (the demod kernel writes the same soft bits again where nothing changed).
static int replay_fic_frames(dabphy_handle* h, const Batch& b)
{
    const uint32_t B = b.B, F = b.F;
    int r;
    SyncArgs sa = sync_args(h, b.cur, F, h->chain_valid[b.cur]);
    // the FIC of ONE frame per step: a class of 4 B code words (frame_sel), decoded into the head of the FIB buffer -- the
    // full-batch FIC pass of decode_batch writes every FIB again
    const VitClass c = fic_class(h, (int)(B * 4));
    CrcArgs k = crc_args(h, b);
    // (state-parallel when 4 B code words are few: a replayed frame then costs a twentieth of a 774-step lane-per-code-word launch;
    // the class is the same for every frame, only the frame selector moves)
    FicOneClass fic;
    if ((r = fic_one_prepare(h, fic, fic_gather_args(h, b, c), h->stream))) return r;
    for (uint32_t f = 0; f < F; f++) {
        sa.frame = (int)f;
        launch_sync_find(sa, h->stream);
        launch_sync_finish(sa, h->stream);
        DemodArgs d1 = b.da; d1.frame_first = (int)f; d1.frame_count = 1; d1.con = nullptr; d1.osc_stats = nullptr;
        d1.chunk_count = (3 + b.da.chunk_len - 1) / b.da.chunk_len;          // the chunks that hold the FIC symbols 1..3 (demod_chunk may be 1 or 2)
        launch_demod(d1, (int)B, h->stream);
        k.frame_sel = (int)f + 1;
        fic_one_launch(h, fic, (int)f + 1, h->stream);
        launch_fib_crc(k, h->stream);
        CrcArgs kf = k; kf.frame_sel = 0; kf.frame_first = (int)f; kf.frame_count = 1;
        launch_fic_ratio(kf, h->stream);
    }
    return 0;
}

// Pipelined modes: the chains of the NEXT batch(es) (40 launches each) are handed to the driver after this batch's decode kernels, so
// that the main stream never waits for the host, and start on the device
//   pipeline_sync = 1: when this batch's demod kernel has finished (event gate).  The FFT stage then runs at its own speed and the
//                      chain shares the device with the Viterbi / RS kernels;
//   pipeline_sync = 2: at once.  Chain and demod kernel share the device: the FFT stage is slower, the chain done earlier;
//   pipeline_sync = 3: gated like 1, but TWO batches ahead: the chain of batch k + 2 is queued while batch k is decoded, so the one
//                      placement stall it meets per step is off the decoder's critical path.
// DESIGN.md section 4.3 has the numbers.
static int queue_next_chains(dabphy_handle* h, const Batch& b)
{
    int r;
    if (h->cfg.pipeline_sync != 2) HIPCHK(h, hipStreamWaitEvent(h->sync_stream, h->ev_chain_gate, 0));
    if (b.depth == 2 && h->ahead < 1 + b.depth && (r = sf_wait_for_pass(h, h->sync_stream))) return r;
    for (; h->ahead < 1 + b.depth; h->ahead++) if ((r = queue_chain(h, (b.cur + h->ahead) % dabphy_handle::N_DESC, b.F))) return r;
    return 0;
}

// SNR + FIC + TII beside the MSC decode, on the auxiliary stream.  The FIC's 4 code words per frame ride in the fused launch
// (dabphy_fused.hip) unless that is switched off; then -- B*F/16 wavefronts of 774 serial trellis steps -- they are decoded here,
// by their own gather + Viterbi pair that fills execution slots beside the MSC classes.
static int queue_aux_work(dabphy_handle* h, const Batch& b)
{
    const uint32_t B = b.B, F = b.F;
    hipStream_t fs = h->aux_stream;
    SnrArgs sn{}; sn.state = h->d_dec; sn.desc = b.d_desc; sn.n_ens = (int)B; sn.n_frames = (int)F; sn.prs_mag = b.da.prs_mag; sn.snr_out = h->s_snr.as<float>();
    const bool snr_main = (h->stream_layout & 16) != 0;
    if (snr_main) { mark(h, dabphy_handle::ST_SNR, false); launch_snr(sn, h->stream); mark(h, dabphy_handle::ST_SNR, true); }
    HIPCHK(h, hipEventRecord(h->ev_demod_done, h->stream));
    HIPCHK(h, hipStreamWaitEvent(fs, h->ev_demod_done, 0));
    // the SNR estimate feeds nothing on the device: off the main stream, so that the MSC decode starts the moment the demod kernel ends
    if (!snr_main) {
        mark(h, dabphy_handle::ST_SNR, false, fs);
        launch_snr(sn, fs);
        mark(h, dabphy_handle::ST_SNR, true, fs);
    }
    if (!h->fplan.fic_in) {
        mark(h, dabphy_handle::ST_FIC, false, fs);
        launch_fic_gather(fic_gather_args(h, b, b.fic), fs);
        launch_viterbi(vit_args(h, b.fic), fs);
    }
    h->tii_ran = false;
    if (h->tii_on) {
        // TII side path (ofdm-processor.cpp:462-466 -> TIIDecoder): needs only the samples and the frame descriptors
        launch_tii(tii_args(h, h->s_iq, h->s_stride, (int64_t)h->s_ring, b.d_desc, B, F), fs);
        h->tii_ran = true;
    }
    // the host's copies of the descriptors and SNR reports leave here, beside the decoder, instead of behind the step's last kernel
    launch_copy_out(b.d_desc, h->h_desc, (size_t)B * F * sizeof(FrameDesc), fs);      // (kernel stores, not copy-engine packets: k_ingest.hip, launch_copy_out)
    launch_copy_out(h->s_snr.p, h->h_snr, (size_t)B * F * sizeof(float), fs);
    HIPCHK(h, hipEventRecord(h->ev_aux_done, fs));
    return 0;
}

// MSC (+ FIC): every class the plan holds in ONE launch; the stage events bracket all of it
static int launch_fused(dabphy_handle* h, const Batch& b)
{
    h->last_frames = b.F; sf_outputs_go(h);
    if (h->fplan.args.n_work <= 0) return 0;
    FusedArgs fa = h->fplan.args; fa.desc = b.d_desc;
    h->fplan.args = fa; h->fplan.launched = true;
    mark(h, dabphy_handle::ST_MSC_VITERBI, false);
    launch_plan(h, h->stream);
    mark(h, dabphy_handle::ST_MSC_VITERBI, true);
    if (fa.done) launch_copy_out(fa.done + fa.n_work + 1, h->h_tb_gave_up, sizeof(uint32_t), h->stream);
    if (h->fplan.fic_in) HIPCHK(h, hipEventRecord(h->ev_fused_done, h->stream));
    return 0;
}

// FIB CRCs, the FIC success ratio (and with it the verdict of exact batch mode), the host's copies of both.  With the FIC in the
// fused launch they wait for nothing but that launch, on a stream of their own: the SNR sums (2048 short waves that feed nothing
// on the device and find no slot while the persistent decoder waves hold them all) must not stand in front of the FIC verdict
static int queue_fic_verdict(dabphy_handle* h, const Batch& b, bool replay)
{
    hipStream_t fs = h->aux_stream;
    if (h->fplan.fic_in) { fs = h->fic_stream; HIPCHK(h, hipStreamWaitEvent(fs, h->ev_fused_done, 0)); mark(h, dabphy_handle::ST_FIC, false, fs); }
    CrcArgs k = crc_args(h, b);
    launch_fib_crc(k, fs);
    k.any_effective = h->d_any_eff;
    if (!replay) launch_fic_ratio(k, fs);                    // (the second pass of exact batch mode has advanced the ratio frame by frame)
    launch_copy_out(h->d_any_eff, h->h_any_eff, sizeof(int32_t), fs);
    mark(h, dabphy_handle::ST_FIC, true, fs);
    launch_copy_out(h->s_fib.p, h->h_fib, (size_t)b.B * b.F * 384, fs);
    launch_copy_out(h->s_ok.p, h->h_ok, (size_t)b.B * b.F * 12, fs);
    HIPCHK(h, hipEventRecord(h->ev_fic_done, fs));
    return 0;
}

// classes the fused launch does not take (DABPHY_FUSED_MSC=0, a window schedule the kernel cannot follow, a span beyond 4 GiB): two
// kernels each, one class after the other (they share the Viterbi scratch)
static int decode_unfused_classes(dabphy_handle* h, const Batch& b)
{
    bool first_two = true;
    int r;
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        if (in_fused_launch(h, ci)) continue;
        auto& cls = h->classes[ci];
        if (debug_env("DABPHY_DEBUG")) fprintf(stderr, "dabphy: class %zu (%d bits) through k_msc_gather + k_viterbi\n", ci, cls.prot.nbits);
        VitClass c{};
        const int P = (int)cls.pairs.size();
        if ((r = prepare_class(h, c, cls.prot.nbits, (int)(4 * b.F * (uint32_t)P), 1))) return r;
        c.out = cls.out.as<uint8_t>();
        MscGatherArgs g{}; g.soft = b.da.soft; g.soft_ring = b.ring_frames; g.soft_ens_stride = b.ens_stride; g.state = h->d_state; g.n_ens = (int)b.B; g.n_frames = (int)b.F;
        g.map = cls.map.as<map_t>(); g.pairs = cls.pair_tab.as<MscPair>(); g.tiles = cls.tiles.as<int32_t>(); g.n_pairs = P; g.desc = b.d_desc; g.c = c;
        if (first_two) mark(h, dabphy_handle::ST_MSC_GATHER, false);
        launch_msc_gather(g, h->stream);
        launch_viterbi(vit_args(h, c), h->stream);
        first_two = false;
    }
    if (!first_two) mark(h, dabphy_handle::ST_MSC_GATHER, true);       // (gather + decode pairs of all such classes)
    return 0;
}

// The decode of the batch whose descriptors are in b.d_desc.  `replay` = the second pass of exact batch mode.
static int decode_batch(dabphy_handle* h, Batch& b, const bool replay)
{
    int r;
    if (replay && (r = replay_fic_frames(h, b))) return r;
    mark(h, dabphy_handle::ST_DEMOD, false);
    launch_demod(b.da, (int)b.B, h->stream);
    tick(h, b, 2);
    mark(h, dabphy_handle::ST_DEMOD, true);
    if (!replay && (h->cfg.pipeline_sync == 1 || h->cfg.pipeline_sync == 3)) HIPCHK(h, hipEventRecord(h->ev_chain_gate, h->stream));
    // (cfg.sync_early: in front of the decoder (0, the default: neutral on the headline, 0.2 ms on a batch of drifting ensembles, whose
    // window searches run one after the other in the find chain -- latency-bound work for one work-group per ensemble that belongs beside the
    // decoder); behind it (1); in front only while the last pass met ensembles whose window moves (2); 3: an experiment, see below)
    if (!replay && b.depth == 2 && (r = sf_launch_waiting(h))) return r;
    const bool early = h->chain_early || (h->cfg.pipeline_sync != 2 && (h->cfg.sync_early == 0 || h->cfg.sync_early == 3 || (h->cfg.sync_early == 2 && h->drift_seen)));
    if (!replay && b.depth && early) {
        // the next batch's synchroniser is handed to the device BEFORE this batch's decoder (whose persistent waves would otherwise hold
        // every wave slot until the end of the step: the synchroniser then runs in the step's tail)
        h->wide_front_recorded = false;
        if ((r = queue_next_chains(h, b))) return r;
        // (sync_early 3: which of the two launches that become ready with the demod kernel's end gets the wave slots is the hardware's
        // choice -- the decoder's persistent waves, once resident, give none back --: the decoder's launch waits for the wide pass
        // proper, ~0.8 ms of throughput work that then has the device to itself; the find chain's rounds run beside the decoder)
        if (h->cfg.sync_early == 3 && h->wide_front_recorded) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_wide_front, 0));
    }
    if (!replay && (r = sf_launch_waiting(h))) return r;       // (dabphy_set_auto_superframes(2): the PREVIOUS batch's filter pass)
    if ((r = sf_wait_for_pass(h, h->stream))) return r;
    if ((r = queue_aux_work(h, b))) return r;
    // pairs selected since the last batch learn the CIF count they start at (their time de-interleaver fills from here, dab-audio.cpp:146-149)
    for (auto& cls : h->classes) if (cls.cif0_pending) launch_pair_cif0(cls.pair_tab.as<MscPair>(), (int)cls.pairs.size(), b.d_desc, (int)b.F, h->stream);
    if ((r = launch_fused(h, b))) return r;
    if ((r = queue_fic_verdict(h, b, replay))) return r;
    if ((r = decode_unfused_classes(h, b))) return r;
    if ((r = sf_inline_pass(h))) return r;
    if (h->mp2_auto && (r = launch_mp2_pass(h, b.F))) return r;
    return DABPHY_OK;
}

// the main stream joins the FIC verdict and the auxiliary work; the host waits for the batch
static int finish_pass(dabphy_handle* h)
{
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fic_done, 0));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_aux_done, 0));
    return 0;
}

// Exact batch mode: a coarse-corrector decision of this batch was taken with a stale FIC ratio and can have mattered.  Everything
// the batch changed is put back (restore_carried; the soft-bit ring and the outputs are simply written again) and the batch is
// decoded a second time with the feedback the reference has; the chains that ran ahead on the wrong state are queued again behind it.
static int replay_batch(dabphy_handle* h, Batch& b)
{
    int r;
    HIPCHK(h, hipStreamSynchronize(h->sync_stream));
    HIPCHK(h, hipStreamSynchronize(h->aux_stream));
    HIPCHK(h, hipStreamSynchronize(h->fic_stream));
    for (int i = 0; i < dabphy_handle::N_DESC; i++) h->wide_pending[i] = false;
    if ((r = restore_carried(h, b.cur))) return r;
    if ((r = decode_batch(h, b, true))) return r;
    if ((r = finish_pass(h))) return r;
    if ((r = chanber_pass(h, b.d_desc, b.F))) return r;       // (the counts of the first pass are replaced: they belong to the bytes the getters return)
    if ((r = sync(h))) return r;
    // the batches synchronised ahead started from the state the first pass left: again, from the right one.  (The chain reads the
    // FIC ratio: the main stream has just been drained.)
    for (int i = 1; i <= b.depth; i++) if ((r = queue_chain(h, (b.cur + i) % dabphy_handle::N_DESC, b.F))) return r;
    h->n_replayed_batches++;
    return 0;
}

// split traceback: walkers that gave up on a group's flag (k_viterbi.hip: tb_consume) would have decoded garbage -- never silently
// (the counter came back with the batch: a copy queued behind the launch, in front of the call's final synchronisation)
static int check_split_traceback(dabphy_handle* h)
{
    if (!(h->fplan.args.done && h->fplan.launched && !h->fplan.use_sp)) return 0;
    if (h->h_tb_gave_up && *h->h_tb_gave_up) { h->err = "split traceback: " + std::to_string(*h->h_tb_gave_up) + " groups were walked back without their decisions having been published"; return DABPHY_ERR_HIP; }
    return 0;
}

static void report_timeline(dabphy_handle* h, const Batch& b)
{
    HostTimeline& tl = h->tl;
    for (int i = 0; i < 5; i++) tl.acc[i] += b.t[i];
    tl.n++;
    if (tl.n % 8 == 0) fprintf(stderr, "dabphy timing [us]: before resolve %.1f, resolved %.1f, demod launched %.1f, all launched %.1f, synced %.1f (n=%ld)\n", tl.acc[0] / tl.n, tl.acc[1] / tl.n, tl.acc[2] / tl.n, tl.acc[3] / tl.n, tl.acc[4] / tl.n, tl.n);
}

extern "C" {

// One batch: acquisition where needed, n_frames frame steps of the synchroniser, then the fully parallel stages.
int dabphy_process(dabphy_handle* h, uint32_t n_frames)
{
    DeviceBind dev_(h);
    if (!h || n_frames == 0 || n_frames > h->cfg.max_frames) return DABPHY_ERR_INVALID;
    if (h->tl_on < 0) h->tl_on = debug_env("DABPHY_DEBUG_TIMING") ? 1 : 0;
    Batch b;
    b.t0 = h->tl_on ? now_us() : 0.0;
    if (!h->s_iq) { h->err = "no sample stream bound"; return DABPHY_ERR_STATE; }
    const uint32_t F = b.F = n_frames;
    b.B = h->cfg.n_ensembles; b.ring_frames = (int)h->cfg.max_frames + 5; b.ens_stride = soft_ens_stride(h);
    int r;
    if ((r = sf_batch_begins(h, n_frames))) return r;        // (a deferred filter pass of the last batch that cannot wait any longer)
    if ((r = apply_subchannels(h))) return r;                // per-ensemble sub-channel changes since the last batch (dabphy_set_subchannels_ensemble)
    if ((r = apply_audio_kinds(h))) return r;                // ... and audio kinds (dabphy_set_audio_kinds_ensemble)
    if ((r = reserve_batch(h, b))) return r;
    h->soft_ring = b.ring_frames;
    for (int i = 0; i < dabphy_handle::ST_COUNT; i++) h->ev_used[i] = false;
    if (h->presynced != 0 && h->presynced != F) { h->err = "pipelined mode needs a constant n_frames"; return DABPHY_ERR_STATE; }
    if ((r = wait_for_ingest(h))) return r;
    b.depth = h->cfg.pipeline_sync == 3 ? 2 : (h->cfg.pipeline_sync ? 1 : 0);
    const int cur = b.cur = h->desc_sel;
    if (h->ahead == 0) {
        // the previous batch's decoder results (FIC ratio) must be final before the chain consults them
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((r = queue_chain(h, cur, F))) return r;
        h->ahead = 1;
    }
    tick(h, b, 0);
    if ((r = resolve_chain(h, cur))) return r;
    tick(h, b, 1);
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_chain_end[cur], 0));      // this batch's chain only: later ones may still be running
    h->presynced = b.depth ? F : 0;
    b.d_desc = h->s_desc2[cur].as<FrameDesc>();
    h->last_desc = b.d_desc;
    h->cur_cir = h->cfg.want_impulse_response ? h->s_cir2[cur].as<float>() : nullptr;
    b.da = demod_args(h, b);
    b.fic = fic_class(h, (int)(b.B * F * 4));

    if (replay_armed(h, F) && (r = save_carried(h))) return r;
    h->mp2_done = false;                                     // (this batch's MP2 pass: in decode_batch with dabphy_set_auto_mp2, else the first getter's)
    if ((r = decode_batch(h, b, false))) return r;
    if (b.depth && (r = queue_next_chains(h, b))) return r;  // (behind the decoder, unless decode_batch queued them in front of it)
    h->desc_sel = (cur + 1) % dabphy_handle::N_DESC; h->ahead--;
    if ((r = finish_pass(h))) return r;
    if ((r = chanber_pass(h, b.d_desc, F))) return r;         // dabphy_set_channel_ber: behind every decoder of the batch, in front of the wait below (dabphy_chanber.hip: "Order")
    tick(h, b, 3);
    if ((r = sync(h))) return r;
    tick(h, b, 4);
    if (replay_armed(h, F) && *h->h_any_eff && (r = replay_batch(h, b))) return r;

    sf_batch_decoded(h, b.d_desc, F);
    // the host's mirror of the pair tables follows what k_pair_cif0 wrote (same rule, from the host's copy of the descriptors)
    for (auto& cls : h->classes) if (cls.cif0_pending) {
        for (MscPair& p : cls.pairs) if (p.cif0 < 0) p.cif0 = 4 * h->h_desc[(size_t)p.ens * F].frame_no;
        cls.cif0_pending = false;
    }
    if ((r = check_split_traceback(h))) return r;
    if (h->tl_on) report_timeline(h, b);
    { float t = 0; h->chain_ms = (hipEventElapsedTime(&t, h->ev_chain_beg[cur], h->ev_chain_end[cur]) == hipSuccess) ? t : 0.0f; }
    return DABPHY_OK;
}

} // extern "C"
