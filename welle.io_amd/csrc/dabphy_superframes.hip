// welle.io_amd/csrc/dabphy_superframes.hip -- Reed-Solomon seams (RSDecoder::DecodeSuperframe) and the DAB+ superframe filter (SuperframeFilter::Feed) of a batch.
// (split from dabphy_api.hip in round 3; dabphy_internal.h has the map of the translation units)
#include "dabphy_internal.h"

namespace {
// The code's tables (dabphy_kernels.h: RS_GF_BYTES, RS_GTAB_BYTES), built once, thread-safely: the node receiver creates its handles from several
// host threads.  GF(256) of RS(120,110), field polynomial 0x11D (init_rs.h:48-60): alpha_to[256], index_of[256]; then the remainder table of
// the generator polynomial g(x) = prod (x - alpha^i), i = 0 .. 9 (init_rs.h:71-94 with fcr = 0, prim = 1): row f = f g_0 .. f g_9, zeros to 16.
struct RsTables {
    uint8_t b[RS_GF_BYTES + RS_GTAB_BYTES]; bool ok;
    RsTables()
    {
        int sr = 1; memset(b, 0, sizeof b); b[256 + 0] = 255; b[255] = 0;
        for (int i = 0; i < 255; i++) { b[256 + sr] = (uint8_t)i; b[i] = (uint8_t)sr; sr <<= 1; if (sr & 256) sr ^= 0x11D; sr &= 255; }
        const uint8_t* alpha_to = b; const uint8_t* index_of = b + 256;
        auto mul = [&](int x, int y) { return x && y ? (int)alpha_to[(index_of[x] + index_of[y]) % 255] : 0; };
        int g[11] = {1};                                                    // g <- g (x + alpha^i), coefficient of x^k in g[k]
        for (int i = 0; i < 10; i++) for (int k = i + 1; k >= 0; k--) g[k] = (k ? g[k - 1] : 0) ^ mul(g[k], alpha_to[i]);
        for (int f = 0; f < 256; f++) for (int k = 0; k < 10; k++) b[RS_GF_BYTES + 16 * f + k] = (uint8_t)mul(f, g[k]);
        // the row of f = 1 is g itself, g is monic of degree 10 and vanishes at alpha^0 .. alpha^9
        ok = g[10] == 1;
        for (int k = 0; k < 16; k++) ok = ok && b[RS_GF_BYTES + 16 + k] == (k < 10 ? g[k] : 0);
        for (int i = 0; i < 10; i++) { int v = 0; for (int k = 10; k >= 0; k--) v = mul(v, alpha_to[i]) ^ g[k]; ok = ok && v == 0; }
    }
};
}

extern "C" {

static int ensure_rs_tables(dabphy_handle* h)
{
    if (h->sf_gf.p) return 0;
    static const RsTables tab;
    if (!tab.ok) { h->err = "Reed-Solomon generator polynomial: table self-check failed"; return DABPHY_ERR_STATE; }
    const size_t bytes = RS_WIDE_STATS_OFF + 2 * sizeof(unsigned long long);      // + the wide pass' two counters
    int r;
    if ((r = ensure(h, h->sf_gf, bytes))) return r;
    HIPCHK(h, hipMemsetAsync(h->sf_gf.p, 0, bytes, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->sf_gf.p, tab.b, sizeof tab.b, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// Device buffers of the superframe filter for F frames per batch: every DAB+-rate class gets its own region of the event / count /
// superframe / verdict buffers (all classes of a bucket run in one launch); the window state of a class is created with the class
// (apply_subchannels, which also carries the windows of the services that stay).
int prepare_superframes(dabphy_handle* h, uint32_t F)
{
    const int n_cif = (int)(4 * F), n_slots = n_cif / 5 + 1;
    size_t pairs = 0, bytes = 0;
    int r;
    for (auto& cls : h->classes) {
        if (!cls.dabplus_rate()) continue;
        const size_t P = cls.pairs.size();
        cls.sf_pair0 = pairs; cls.sf_bytes0 = bytes;
        pairs += P; bytes += P * n_slots * 5 * (size_t)(cls.prot.nbits / 8);
        if (cls.sf_state.cap < cls.sf_stride() * P) {
            if ((r = ensure(h, cls.sf_state, cls.sf_stride() * P))) return r;
            HIPCHK(h, hipMemsetAsync(cls.sf_state.p, 0, cls.sf_state.cap, h->stream));      // sf_state_count = 0: nothing collected yet
        }
    }
    if (!pairs) return 0;
    if ((r = ensure(h, h->sf_events, sizeof(SfEvent) * pairs * n_cif))) return r;
    if ((r = ensure(h, h->sf_count, sizeof(int32_t) * pairs))) return r;
    if ((r = ensure(h, h->sf_bytes, bytes))) return r;
    if ((r = ensure(h, h->sf_accept, sizeof(int32_t) * pairs))) return r;
    if ((r = ensure(h, h->sf_batch, SF_BATCH_BYTES))) return r;
    if (!h->h_sf_batch && (r = pinned_alloc(h, SF_BATCH_BYTES, &h->h_sf_batch))) return r;
    return ensure_rs_tables(h);
}


int dabphy_rs_superframes(dabphy_handle* h, uint8_t* sf, uint32_t s_per_sf, uint32_t n_sf, int32_t* corrected, int32_t* uncorrectable)
{
    DeviceBind dev_(h);
    if (!h || !sf || !corrected || !uncorrectable || s_per_sf == 0 || n_sf == 0) return DABPHY_ERR_INVALID;
    const size_t bytes = (size_t)120 * s_per_sf * n_sf;
    int r;
    if ((r = ensure(h, h->in8, bytes))) return r;
    if ((r = ensure(h, h->rs_result, 2 * sizeof(int) * n_sf))) return r;
    if ((r = ensure_rs_tables(h))) return r;
    HIPCHK(h, hipMemcpyAsync(h->in8.p, sf, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->rs_result.p, 0, 2 * sizeof(int) * n_sf, h->stream));
    RsArgs a{}; a.data = h->in8.as<uint8_t>(); a.sf_stride = (size_t)120 * s_per_sf; a.n_sf = (int)n_sf; a.s = (int)s_per_sf;
    a.corr = h->rs_result.as<int>(); a.uncorr = h->rs_result.as<int>() + n_sf; a.gf = h->sf_gf.as<uint8_t>();
    launch_rs_superframes(a, h->stream);
    HIPCHK(h, hipMemcpyAsync(sf, h->in8.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(corrected, a.corr, sizeof(int) * n_sf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(uncorrectable, a.uncorr, sizeof(int) * n_sf, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

int dabphy_rs_decode_msc(dabphy_handle* h, int32_t subch_index, const int32_t* first_cif, int32_t* corrected, int32_t* uncorrectable)
{
    DeviceBind dev_(h);
    if (!h || !first_cif || !h->last_frames) return DABPHY_ERR_INVALID;
    const uint32_t B = h->cfg.n_ensembles, F = h->last_frames;
    const int n_cif = (int)(4 * F), n_sf = n_cif / 5 + 1;
    int r;
    if ((r = ensure(h, h->rs_first, sizeof(int) * B))) return r;
    if ((r = ensure_rs_tables(h))) return r;
    HIPCHK(h, hipMemcpyAsync(h->rs_first.p, first_cif, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
    if (corrected) memset(corrected, 0, sizeof(int32_t) * B);
    if (uncorrectable) memset(uncorrectable, 0, sizeof(int32_t) * B);
    // Per pair the rows that hold this batch's logical frames (dabphy_get_msc); a pair the call leaves out gets an empty range: another list
    // position than the one asked for, or an MP2 service -- its bytes are no Reed-Solomon code words (dabphy_set_audio_kinds_ensemble)
    bool first_launch = true, any = subch_index < 0, any_at_index = false;
    std::vector<std::vector<int2>> rows_of(h->classes.size());       // (host sources of queued copies: they live until the stream has been synchronised)
    for (auto& cls : h->classes) {
        const int bitrate = cls.prot.nbits / 24;
        const size_t P = cls.pairs.size(), nres = P * n_sf * 2;
        std::vector<int2>& rows = rows_of[&cls - h->classes.data()];
        rows.assign(P, make_int2(0, 0));
        bool work = false;
        for (size_t p = 0; p < P; p++) {
            const MscPair& pp = cls.pairs[p];
            if (subch_index >= 0 && pp.idx != subch_index) continue;
            any_at_index = true;
            if (cls.kind[p] == DABPHY_AUDIO_MP2) continue;
            any = true;
            dabphy_handle::PairRef w; w.cls = (int)(&cls - h->classes.data()); w.pair = (int)p;
            msc_rows_info(h, (uint32_t)pp.ens, w, &rows[p].x, &rows[p].y);
            work |= rows[p].x < rows[p].y;
        }
        if (bitrate % 8 || !work) continue;
        if ((r = ensure(h, h->rs_result, nres * sizeof(int)))) return r;
        if ((r = ensure(h, h->rs_rows, P * sizeof(int2)))) return r;
        HIPCHK(h, hipMemsetAsync(h->rs_result.p, 0, nres * sizeof(int), h->stream));
        HIPCHK(h, hipMemcpyAsync(h->rs_rows.p, rows.data(), P * sizeof(int2), hipMemcpyHostToDevice, h->stream));
        RsMscArgs a{}; a.out = cls.out.as<uint8_t>(); a.n_cif = n_cif; a.n_pairs = (int)P; a.pairs = cls.pair_tab.as<MscPair>();
        a.frame_bytes = cls.prot.nbits / 8; a.s = bitrate / 8; a.n_sf_per_pair = n_sf; a.rows = h->rs_rows.as<int2>();
        a.first_cif = h->rs_first.as<int>(); a.result = h->rs_result.as<int>(); a.gf = h->sf_gf.as<uint8_t>();
        if (h->profiling && first_launch) { hipError_t e = hipEventRecord(h->ev_beg[dabphy_handle::ST_RS], h->stream); (void)e; }
        launch_rs_msc(a, h->stream);
        if (h->profiling && first_launch) { hipError_t e = hipEventRecord(h->ev_end[dabphy_handle::ST_RS], h->stream); (void)e; h->ev_used[dabphy_handle::ST_RS] = true; }
        first_launch = false;
        if (corrected || uncorrectable) {
            std::vector<int> res(nres);
            HIPCHK(h, hipMemcpyAsync(res.data(), h->rs_result.p, nres * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            if ((r = sync(h))) return r;
            for (size_t p = 0; p < P; p++)
                for (int q = 0; q < n_sf; q++) {
                    const size_t o = (p * n_sf + q) * 2;                            // [pair][superframe]
                    if (corrected) corrected[cls.pairs[p].ens] += res[o];
                    if (uncorrectable) uncorrectable[cls.pairs[p].ens] += res[o + 1];
                }
        }
    }
    if (!any) {                                                      // no ensemble has a sub-channel at that position, or only MP2 services
        h->err = any_at_index ? "the sub-channel at this position is an MP2 service in every ensemble that has one" : "no ensemble has a sub-channel at this position";
        r = sync(h);
        return r ? r : DABPHY_ERR_INVALID;
    }
    return sync(h);
}

// The filter over a selection of classes: sel[i] = (class, DEVICE list of its pairs to walk or nullptr for all of them, how many).  The
// classes of a bucket (kernel LDS size) go in ONE launch each of the wide pass, the verdict and the serial walk; their argument blocks
// travel through a page-locked staging area that the caller must not reuse before the stream has been synchronised (every caller
// synchronises before it returns, dabphy_process at its end).
static int run_superframes(dabphy_handle* h, const std::vector<SfSel>& sel, int32_t* stats, hipStream_t st, const FrameDesc* desc, uint32_t F)
{
    const int n_cif = (int)(4 * F), n_slots = n_cif / 5 + 1;        // (desc, F: a deferred pass names the batch it belongs to, the handle has moved on)
    int r;
    if ((r = prepare_superframes(h, F))) return r;
    if (!h->sf_batch.p) return 0;                                        // no DAB+-rate class at all
    // staging layout per bucket: [SF_BATCH_CLASSES argument blocks][SF_BATCH_CLASSES + 1 first blocks]
    uint8_t* const hs = reinterpret_cast<uint8_t*>(h->h_sf_batch);
    uint8_t* const ds = h->sf_batch.as<uint8_t>();
    constexpr size_t BUCKET = SF_BATCH_BYTES / 3, FIRST0 = SF_BATCH_CLASSES * sizeof(SfArgs);
    int n_in[3] = {0, 0, 0}, blocks[3] = {0, 0, 0}, max_s[3] = {0, 0, 0};
    for (const SfSel& e : sel) {
        auto& cls = h->classes[e.cls];
        if (!cls.dabplus_rate() || cls.pairs.empty()) continue;
        const int bitrate = cls.prot.nbits / 24, fb = cls.prot.nbits / 8, bk = sf_bucket(fb);
        SfArgs a{};
        a.out = cls.out.as<uint8_t>(); a.n_cif = n_cif; a.n_pairs = (int)cls.pairs.size(); a.pairs = cls.pair_tab.as<MscPair>(); a.frame_bytes = fb;
        a.run = e.d_run; a.n_run = e.d_run ? e.n_run : a.n_pairs;
        if (a.n_run <= 0) continue;
        a.s = bitrate / 8; a.desc = desc; a.n_frames = (int)F;
        a.state = cls.sf_state.as<uint8_t>(); a.state_stride = cls.sf_stride();
        a.events = h->sf_events.as<SfEvent>() + cls.sf_pair0 * n_cif; a.n_events = h->sf_count.as<int32_t>() + cls.sf_pair0;
        a.sf = h->sf_bytes.as<uint8_t>() + cls.sf_bytes0; a.n_slots = n_slots; a.stats = stats;
        a.gf = h->sf_gf.as<uint8_t>(); a.accepted = h->sf_accept.as<int32_t>() + cls.sf_pair0;
        a.wide_stats = reinterpret_cast<unsigned long long*>(h->sf_gf.as<uint8_t>() + RS_WIDE_STATS_OFF);
        reinterpret_cast<SfArgs*>(hs + bk * BUCKET)[n_in[bk]] = a;
        reinterpret_cast<int32_t*>(hs + bk * BUCKET + FIRST0)[n_in[bk]] = blocks[bk];
        n_in[bk]++; blocks[bk] += a.n_run; max_s[bk] = std::max(max_s[bk], a.s);
    }
    for (int bk = 0; bk < 3; bk++) {
        if (!n_in[bk]) continue;
        reinterpret_cast<int32_t*>(hs + bk * BUCKET + FIRST0)[n_in[bk]] = blocks[bk];
        HIPCHK(h, hipMemcpyAsync(ds + bk * BUCKET, hs + bk * BUCKET, n_in[bk] * sizeof(SfArgs), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(ds + bk * BUCKET + FIRST0, hs + bk * BUCKET + FIRST0, (n_in[bk] + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    for (int bk = 0; bk < 3; bk++) {
        if (!n_in[bk]) continue;
        SfBatch bt{}; bt.cls = reinterpret_cast<const SfArgs*>(ds + bk * BUCKET); bt.first = reinterpret_cast<const int32_t*>(ds + bk * BUCKET + FIRST0); bt.n_cls = n_in[bk];
        launch_superframe_bucket(bt, bk, blocks[bk], n_cif, max_s[bk], true, st);
    }
    for (int bk = 0; bk < 3; bk++) {                                     // (dabphy_time_superframe_wide)
        auto& w = h->sf_wide_last[bk];
        w.bt = SfBatch{}; w.blocks = n_in[bk] ? blocks[bk] : 0; w.n_cif = n_cif; w.max_s = max_s[bk];
        if (n_in[bk]) { w.bt.cls = reinterpret_cast<const SfArgs*>(ds + bk * BUCKET); w.bt.first = reinterpret_cast<const int32_t*>(ds + bk * BUCKET + FIRST0); w.bt.n_cls = n_in[bk]; w.bt.replay = 1; }
    }
    h->sf_wide_gen = h->buf_gen;
    return 0;
}

namespace {
// The filter over a selection of pairs (class, pair) given per output row; events / counts / superframes of row i land at
// events + i * n_cif, n_events + i, sf + i * n_slots * 5 * fb.  Every selected pair must have frames of fb bytes.
int superframes_of(dabphy_handle* h, const std::vector<dabphy_handle::PairRef>& rows, int fb, dabphy_sf_event* events, int32_t* n_events, uint8_t* sf)
{
    const uint32_t F = h->last_frames;
    const int n_cif = (int)(4 * F), n_slots = n_cif / 5 + 1;
    int r;
    if ((r = prepare_superframes(h, F))) return r;
    std::vector<int32_t> run(rows.size());
    if ((r = ensure(h, h->sf_run, rows.size() * sizeof(int32_t)))) return r;
    std::vector<SfSel> sel; std::vector<std::vector<size_t>> mine_of;
    size_t used = 0;
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        std::vector<size_t> mine;
        for (size_t i = 0; i < rows.size(); i++) if (rows[i].cls == (int)ci) mine.push_back(i);
        if (mine.empty()) continue;
        for (size_t k = 0; k < mine.size(); k++) run[used + k] = rows[mine[k]].pair;
        sel.push_back(SfSel{(int)ci, h->sf_run.as<int32_t>() + used, (int)mine.size()});
        used += mine.size(); mine_of.push_back(std::move(mine));
    }
    HIPCHK(h, hipMemcpyAsync(h->sf_run.p, run.data(), used * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if ((r = run_superframes(h, sel, nullptr, h->stream, h->last_desc, F))) return r;
    for (size_t s = 0; s < sel.size(); s++) {
        const auto& cls = h->classes[sel[s].cls];
        for (size_t i : mine_of[s]) {
            const size_t bm = (size_t)rows[i].pair;
            HIPCHK(h, hipMemcpyAsync(events + i * n_cif, h->sf_events.as<SfEvent>() + (cls.sf_pair0 + bm) * n_cif, sizeof(SfEvent) * n_cif, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(n_events + i, h->sf_count.as<int32_t>() + cls.sf_pair0 + bm, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            if (sf) HIPCHK(h, hipMemcpyAsync(sf + i * n_slots * 5 * fb, h->sf_bytes.as<uint8_t>() + cls.sf_bytes0 + bm * n_slots * 5 * fb, (size_t)n_slots * 5 * fb, hipMemcpyDeviceToHost, h->stream));
        }
    }
    return sync(h);                  // (`run` and the staging area are free again)
}
}

int dabphy_superframes(dabphy_handle* h, uint32_t subch_index, dabphy_sf_event* events, int32_t* n_events, uint8_t* sf)
{
    DeviceBind dev_(h);
    static_assert(sizeof(dabphy_sf_event) == sizeof(SfEvent), "event layouts must match");
    if (!h || !events || !n_events || !h->last_frames || !h->last_desc) return DABPHY_ERR_INVALID;
    const uint32_t B = h->cfg.n_ensembles;
    std::vector<dabphy_handle::PairRef> rows(B);
    int fb = 0;
    for (uint32_t b = 0; b < B; b++) {
        if (subch_index >= h->where[b].size()) { h->err = "ensemble " + std::to_string(b) + " has no sub-channel " + std::to_string(subch_index); return DABPHY_ERR_INVALID; }
        rows[b] = h->where[b][subch_index];
        const auto& cls = h->classes[rows[b].cls];
        if (!cls.dabplus_rate()) { h->err = "sub-channel bit rate is not a DAB+ rate"; return DABPHY_ERR_INVALID; }
        if (cls.kind[rows[b].pair] == DABPHY_AUDIO_MP2) { h->err = "ensemble " + std::to_string(b) + ": the sub-channel is an MP2 service"; return DABPHY_ERR_INVALID; }
        if (fb && fb != cls.prot.nbits / 8) { h->err = "the ensembles' sub-channels at this position differ in bit rate: use dabphy_superframes_ensemble"; return DABPHY_ERR_INVALID; }
        fb = cls.prot.nbits / 8;
    }
    return superframes_of(h, rows, fb, events, n_events, sf);
}

int dabphy_superframes_ensemble(dabphy_handle* h, uint32_t ensemble, uint32_t subch_index, dabphy_sf_event* events, int32_t* n_events, uint8_t* sf)
{
    DeviceBind dev_(h);
    if (!h || !events || !n_events || !h->last_frames || !h->last_desc || ensemble >= h->cfg.n_ensembles || subch_index >= h->where[ensemble].size()) return DABPHY_ERR_INVALID;
    const std::vector<dabphy_handle::PairRef> rows(1, h->where[ensemble][subch_index]);
    const auto& cls = h->classes[rows[0].cls];
    if (!cls.dabplus_rate()) { h->err = "sub-channel bit rate is not a DAB+ rate"; return DABPHY_ERR_INVALID; }
    if (cls.kind[rows[0].pair] == DABPHY_AUDIO_MP2) { h->err = "the sub-channel is an MP2 service (dabphy_set_audio_kinds_ensemble)"; return DABPHY_ERR_INVALID; }
    return superframes_of(h, rows, cls.prot.nbits / 8, events, n_events, sf);
}

namespace {
using SfPass = dabphy_handle::SfPass;
static size_t sf_totals_bytes(const dabphy_handle* h) { return sizeof(int32_t) * 4 * h->cfg.n_ensembles; }
// SuperframeFilter over every DAB+ sub-channel of every ensemble, totals into sf_stats: over the last batch on the main stream, or -- deferred -- over the batch that waits in h->sf on the auxiliary stream
static int launch_superframe_stats(dabphy_handle* h, bool deferred = false)
{
    hipStream_t st = deferred ? h->aux_stream : h->stream; int r;
    if ((r = ensure(h, h->sf_stats, sf_totals_bytes(h)))) return r;
    HIPCHK(h, hipMemsetAsync(h->sf_stats.p, 0, sf_totals_bytes(h), st));
    std::vector<SfSel> sel;
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        const auto& c = h->classes[ci];
        if (!c.dabplus_rate()) continue;
        if (!c.n_mp2) sel.push_back(SfSel{(int)ci, nullptr, 0});
        else if (c.n_dab) sel.push_back(SfSel{(int)ci, c.dab_run.as<int32_t>(), c.n_dab});      // (MP2 services are left out: dabphy_mp2.hip)
    }
    if (sel.empty()) return 0;
    if (h->profiling) { hipError_t e = hipEventRecord(h->ev_beg[dabphy_handle::ST_RS], st); (void)e; }
    if ((r = run_superframes(h, sel, h->sf_stats.as<int32_t>(), st, deferred ? h->sf.desc : h->last_desc, deferred ? h->sf.frames : h->last_frames))) return r;
    if (h->profiling) { hipError_t e = hipEventRecord(h->ev_end[dabphy_handle::ST_RS], st); (void)e; h->ev_used[dabphy_handle::ST_RS] = true; }
    return au_pack_pass(h, sel, st, deferred ? h->sf.frames : h->last_frames);       // (dabphy_set_au_drain; nothing while it is off)
}
// the host waits for a pass in flight: its totals are in h_sf_stats
static int land_totals(dabphy_handle* h) { if (h->sf.totals == SfPass::IN_FLIGHT) { HIPCHK(h, hipEventSynchronize(h->sf.done)); h->sf.totals = SfPass::LANDED; } return DABPHY_OK; }
}

// ---- the filter as a pass of dabphy_process (dabphy_set_auto_superframes).  Every access to h->sf is below; dabphy_internal.h has the table.
bool sf_pass_on(const dabphy_handle* h) { return h->sf.mode != SfPass::OFF; }
bool sf_windows_carried(const dabphy_handle* h) { return h->sf.mode != SfPass::DEFERRED; }     // (deferred: this batch's pass has not run when exact batch mode decodes the batch again, nothing to put back)

// Mode 2: the pass of batch k is queued by dabphy_process(k + 1) behind that batch's demod launch, and runs beside the FFT
// stage instead of in the step's tail.  decode_batch calls this twice: two batches ahead in front of the next chains, one of which reuses
// the descriptors the pass reads and has to wait for it; on every schedule in front of the decoders, where nothing is left to launch
// when it went in front of the chains.  (On the AUXILIARY stream, idle until this batch's demod kernel has finished: a stream of its own
// would be the handle's eighth, the runtime multiplexes them onto four hardware queues, and the first version ran behind the demod kernel)
int sf_launch_waiting(dabphy_handle* h)
{
    SfPass& p = h->sf; int r;
    if (!p.desc) return DABPHY_OK;
    if (!p.done && (r = new_event(h, &p.done))) return r;
    if ((r = launch_superframe_stats(h, true))) return r;
    launch_copy_out(h->sf_stats.p, h->h_sf_stats, sf_totals_bytes(h), h->aux_stream);
    HIPCHK(h, hipEventRecord(p.done, h->aux_stream));
    p.desc = nullptr; p.totals = SfPass::IN_FLIGHT;
    return DABPHY_OK;
}
// The main stream waits before this batch's decoders overwrite the class outputs the pass reads.  The synchroniser's stream waits TWO batches ahead -- only then:
// N_DESC = 3 --, when the chain queued next writes the descriptor buffer of the PREVIOUS batch, whose pass reads valid / frame_no from it
int sf_wait_for_pass(dabphy_handle* h, hipStream_t st) { if (h->sf.totals == SfPass::IN_FLIGHT) HIPCHK(h, hipStreamWaitEvent(st, h->sf.done, 0)); return DABPHY_OK; }
// The waiting pass now, and the host waits for it: what it reads is about to change -- audio kinds; the classes, which a batch rebuilds; class outputs of its own depth, which another n_frames may grow (reserve_batch: contents not kept)
int sf_flush(dabphy_handle* h) { const int r = sf_launch_waiting(h); return r ? r : land_totals(h); }
int sf_batch_begins(dabphy_handle* h, uint32_t n_frames) { return h->subch_dirty || n_frames != h->sf.frames ? sf_flush(h) : DABPHY_OK; }
void sf_outputs_go(dabphy_handle* h) { if (h->sf.mode != SfPass::DEFERRED) h->sf.totals = SfPass::EMPTY; }      // (mode 2's totals are the batch before's: they stay)
int sf_inline_pass(dabphy_handle* h)
{
    if (h->sf.mode != SfPass::INLINE) return DABPHY_OK;
    if (int r = launch_superframe_stats(h)) return r;
    launch_copy_out(h->sf_stats.p, h->h_sf_stats, sf_totals_bytes(h), h->stream); h->sf.totals = SfPass::LANDED;       // (once dabphy_process has returned: it ends with the main stream drained)
    return DABPHY_OK;
}
void sf_batch_decoded(dabphy_handle* h, const FrameDesc* desc, uint32_t n_frames)
{
    SfPass& p = h->sf;
    if (p.mode != SfPass::DEFERRED) return;
    if (p.totals == SfPass::IN_FLIGHT) p.totals = SfPass::LANDED;       // (the main stream has waited for the previous batch's pass: its totals are in host memory)
    p.desc = desc; p.frames = n_frames; p.polled = false;               // this batch's pass is the next call's
}
int sf_stream_reset(dabphy_handle* h)       // a deferred pass of the stream that ends here is dropped with it (inline totals stay: no fetch reaches them before the next launch)
{
    SfPass& p = h->sf;
    if (p.done) HIPCHK(h, hipStreamSynchronize(h->aux_stream));
    p.desc = nullptr; p.polled = false; if (p.mode == SfPass::DEFERRED) p.totals = SfPass::EMPTY;
    return DABPHY_OK;
}

int dabphy_set_auto_superframes(dabphy_handle* h, int32_t on)
{
    DeviceBind dev_(h);
    if (!h) return DABPHY_ERR_INVALID;
    SfPass& p = h->sf;
    const SfPass::Mode mode = on == 2 ? SfPass::DEFERRED : on ? SfPass::INLINE : SfPass::OFF;
    if (p.mode == SfPass::DEFERRED && mode != p.mode) {
        // leaving the deferred mode: nothing stays waiting -- the last batch's pass runs now if it has not -- and the mode that follows does not filter
        // the last batch a second time: its totals, unless they have been fetched (then zeros), are what the next dabphy_superframes_stats returns
        int r = sf_flush(h); if (r) return r;
        const bool park = h->last_frames && h->h_sf_stats;
        if (park && p.totals != SfPass::LANDED) memset(h->h_sf_stats, 0, sf_totals_bytes(h));
        p.totals = park ? SfPass::LANDED : SfPass::EMPTY; p.polled = false;
    } else if (mode == SfPass::DEFERRED && mode != p.mode) p.totals = SfPass::EMPTY;     // (inline totals not fetched: mode 2 never returned them, and zeroed them when it was left)
    p.mode = mode;
    return DABPHY_OK;
}

int dabphy_superframes_stats(dabphy_handle* h, int32_t* stats)
{
    DeviceBind dev_(h);
    if (!h || !stats) return DABPHY_ERR_INVALID;
    SfPass& p = h->sf; int r;
    if (p.mode == SfPass::DEFERRED) {      // (needs no batch: zeros when nothing waits or has landed, as after dabphy_reset)
        // the first call after a dabphy_process: the totals of the pass that call queued (the batch BEFORE it), zeros if it queued
        // none.  One more call without a dabphy_process in between: the waiting pass of the last batch runs now (the end of a stream)
        if (p.polled && p.totals == SfPass::EMPTY && (r = sf_launch_waiting(h))) return r;
        p.polled = true; if ((r = land_totals(h))) return r;
    } else if (!h->last_frames || !h->last_desc) return DABPHY_ERR_INVALID;
    else if (p.totals != SfPass::LANDED) {       // manual mode, or one more fetch of a batch: the filter runs, every time (and feeds the same frames again)
        if ((r = launch_superframe_stats(h))) return r;
        HIPCHK(h, hipMemcpyAsync(stats, h->sf_stats.p, sf_totals_bytes(h), hipMemcpyDeviceToHost, h->stream));
        return sync(h);
    }
    if (p.totals == SfPass::LANDED) memcpy(stats, h->h_sf_stats, sf_totals_bytes(h));
    else memset(stats, 0, sf_totals_bytes(h));       // (mode 2 only: no pass was queued)
    p.totals = SfPass::EMPTY;
    return DABPHY_OK;
}

// The wide launches of the last filter pass again, alone on the device.  The pass' settle kernel has moved the windows on since, so the
// repetition runs in the kernel's replay form: it leaves out the one attempt per pair that read frames carried INTO the batch (they are gone) and
// the pairs that were walked, and rewrites the events and superframes of every other attempt with what they hold.
int dabphy_time_superframe_wide(dabphy_handle* h, uint32_t iters, float* ms)
{
    DeviceBind dev_(h);
    if (!h || !ms || iters == 0) return DABPHY_ERR_INVALID;
    int r;
    if ((r = sf_flush(h))) return r;                          // (a deferred pass that waits goes first: it is the last batch's, and it writes the staging area the launches name)
    int total = 0;
    for (const auto& w : h->sf_wide_last) total += w.blocks;
    if (!total || h->sf_wide_gen != h->buf_gen) { h->err = "no superframe filter pass has run with the present buffers"; return DABPHY_ERR_STATE; }
    HIPCHK(h, hipDeviceSynchronize());                       // alone on the device: nothing of the pipeline beside it
    ScopedEvent e0, e1;
    HIPCHK(h, e0.create()); HIPCHK(h, e1.create());
    auto again = [&]() { for (int bk = 0; bk < 3; bk++) { const auto& w = h->sf_wide_last[bk]; launch_superframe_wide(w.bt, bk, w.blocks, w.n_cif, w.max_s, h->stream); } };
    again();
    HIPCHK(h, hipEventRecord(e0, h->stream));
    for (uint32_t i = 0; i < iters; i++) again();
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipEventSynchronize(e1));
    float t = 0; HIPCHK(h, hipEventElapsedTime(&t, e0, e1));
    *ms = t / iters;
    return sync(h);
}

} // extern "C"
