// welle.io_amd/csrc/dabphy_mp2.hip -- classic DAB (MP2) services: audio kinds per list position, the MP2 frame check over a batch
// (k_mp2.hip) and its getters, and the unit entry on host-supplied logical frames.  DESIGN.md section 4.7.
#include "dabphy_internal.h"

size_t mp2_stride() { return (sizeof(Mp2State) + MP2_CARRY + 15) & ~(size_t)15; }

namespace {
int mp2_ev_cap(uint32_t F) { return 2 * (int)(4 * F) + 8; }
}

// The kinds asked for (kind_next) onto the classes of the batch: per pair the applied kind, the device lists of a class's DAB+ and MP2
// pairs (only for a class that has an MP2 pair), fresh parser state for a pair that becomes MP2.  Runs in dabphy_process behind
// apply_subchannels; where no MP2 service is or was selected it touches nothing on the device.
int apply_audio_kinds(dabphy_handle* h)
{
    if (!h->kinds_dirty) return DABPHY_OK;
    h->kinds_dirty = false;
    std::vector<std::vector<int32_t>> want(h->classes.size());
    bool device_work = false;
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        const auto& c = h->classes[ci];
        for (size_t p = 0; p < c.pairs.size(); p++) {
            const std::vector<int32_t>& kn = h->kind_next[c.pairs[p].ens];
            want[ci].push_back((size_t)c.pairs[p].idx < kn.size() ? kn[c.pairs[p].idx] : DABPHY_AUDIO_DABPLUS);
            device_work |= want[ci].back() == DABPHY_AUDIO_MP2;
        }
        device_work |= c.n_mp2 > 0;
    }
    int r;
    if (device_work) {
        if ((r = sf_flush(h))) return r;      // nothing queued may still read the run lists (the deferred DAB+ pass of the last batch: run now, with the kinds it was decoded with)
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    const size_t stride = mp2_stride();
    for (size_t ci = 0; ci < h->classes.size(); ci++) {
        auto& c = h->classes[ci];
        std::vector<int32_t> dab, mp2;
        std::vector<size_t> fresh;
        for (size_t p = 0; p < c.pairs.size(); p++) {
            const int32_t k = want[ci][p];
            if (k == DABPHY_AUDIO_MP2 && c.kind[p] != DABPHY_AUDIO_MP2) fresh.push_back(p);
            c.kind[p] = k;
            (k == DABPHY_AUDIO_MP2 ? mp2 : dab).push_back((int32_t)p);
        }
        c.n_mp2 = (int)mp2.size(); c.n_dab = (int)dab.size();
        if (!c.n_mp2) continue;
        if ((r = ensure(h, c.dab_run, (dab.size() + 1) * sizeof(int32_t)))) return r;
        if ((r = ensure(h, c.mp2_run, mp2.size() * sizeof(int32_t)))) return r;
        if (!dab.empty()) HIPCHK(h, hipMemcpyAsync(c.dab_run.p, dab.data(), dab.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(c.mp2_run.p, mp2.data(), mp2.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        if (c.mp2_state.cap < stride * c.pairs.size()) {
            if ((r = ensure(h, c.mp2_state, stride * c.pairs.size()))) return r;
            HIPCHK(h, hipMemsetAsync(c.mp2_state.p, 0, c.mp2_state.cap, h->stream));
        } else {
            for (size_t p : fresh) HIPCHK(h, hipMemsetAsync(c.mp2_state.as<uint8_t>() + p * stride, 0, stride, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));                       // (the host lists above go out of scope)
    }
    return DABPHY_OK;
}

// Buffers of the MP2 pass for F frames per batch (before dabphy_process queues anything)
int prepare_mp2(dabphy_handle* h, uint32_t F)
{
    const int n_cif = (int)(4 * F), cap = mp2_ev_cap(F);
    int r;
    bool any = false;
    for (auto& c : h->classes) {
        if (!c.n_mp2) continue;
        any = true;
        const size_t P = c.pairs.size();
        if ((r = ensure(h, c.mp2_ev, P * cap * sizeof(Mp2Event)))) return r;
        if ((r = ensure(h, c.mp2_n, P * sizeof(int32_t)))) return r;
        if ((r = ensure(h, c.mp2_err, P * n_cif * sizeof(int32_t)))) return r;
        if ((r = ensure(h, c.mp2_fu, P * sizeof(int32_t)))) return r;
    }
    if (any && (r = ensure(h, h->mp2_stats, sizeof(int32_t) * 4 * h->cfg.n_ensembles))) return r;
    return DABPHY_OK;
}

// The MP2 pass over the last batch on the main stream: every MP2 service of every class, one launch per class
int launch_mp2_pass(dabphy_handle* h, uint32_t F)
{
    const FrameDesc* desc = h->last_desc;
    int r;
    if ((r = prepare_mp2(h, F))) return r;
    if (!h->mp2_stats.p) return DABPHY_OK;
    HIPCHK(h, hipMemsetAsync(h->mp2_stats.p, 0, sizeof(int32_t) * 4 * h->cfg.n_ensembles, h->stream));
    bool first = true;
    for (auto& c : h->classes) {
        if (!c.n_mp2) continue;
        Mp2Args a{};
        a.out = c.out.as<uint8_t>(); a.n_cif = (int)(4 * F); a.frame_bytes = c.prot.nbits / 8;
        a.run = c.mp2_run.as<int32_t>(); a.pairs = c.pair_tab.as<MscPair>(); a.desc = desc; a.n_frames = (int)F;
        a.state = c.mp2_state.as<uint8_t>(); a.state_stride = mp2_stride();
        a.events = c.mp2_ev.as<Mp2Event>(); a.ev_cap = mp2_ev_cap(F); a.n_events = c.mp2_n.as<int32_t>();
        a.frame_errors = c.mp2_err.as<int32_t>(); a.first_unverified = c.mp2_fu.as<int32_t>(); a.stats = h->mp2_stats.as<int32_t>();
        if (h->profiling && first) {
            if (!h->ev_mp2[0]) for (int i = 0; i < 2; i++) { const int rc = new_event(h, &h->ev_mp2[i], true); if (rc) return rc; }
            HIPCHK(h, hipEventRecord(h->ev_mp2[0], h->stream));
        }
        launch_mp2(a, c.n_mp2, h->stream);
        first = false;
    }
    if (h->profiling && !first) { HIPCHK(h, hipEventRecord(h->ev_mp2[1], h->stream)); h->mp2_timed = true; }
    h->mp2_done = true;
    return DABPHY_OK;
}

extern "C" {

int dabphy_set_audio_kinds_ensemble(dabphy_handle* h, uint32_t ensemble, const int32_t* kinds, uint32_t n)
{
    if (!h || ensemble >= h->cfg.n_ensembles || (n && !kinds)) return DABPHY_ERR_INVALID;
    if (n != h->subch_next[ensemble].size()) { h->err = "kinds: n must be the length of the ensemble's list as last set"; return DABPHY_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++)
        if (kinds[i] != DABPHY_AUDIO_DABPLUS && kinds[i] != DABPHY_AUDIO_MP2) { h->err = "kinds: DABPHY_AUDIO_DABPLUS or DABPHY_AUDIO_MP2"; return DABPHY_ERR_INVALID; }
    h->kind_next[ensemble].assign(kinds, kinds + n);
    h->kinds_dirty = true;
    return DABPHY_OK;
}

int dabphy_set_auto_mp2(dabphy_handle* h, int32_t on)
{
    if (!h || on < 0 || on > 1) return DABPHY_ERR_INVALID;
    h->mp2_auto = on != 0;
    return DABPHY_OK;
}

int dabphy_mp2_stats(dabphy_handle* h, int32_t* stats)
{
    DeviceBind dev_(h);
    if (!h || !stats || !h->last_frames || !h->last_desc) return DABPHY_ERR_INVALID;
    const uint32_t B = h->cfg.n_ensembles;
    int r;
    if (!h->mp2_done && (r = launch_mp2_pass(h, h->last_frames))) return r;
    if (!h->mp2_stats.p) { memset(stats, 0, sizeof(int32_t) * 4 * B); return DABPHY_OK; }
    HIPCHK(h, hipMemcpyAsync(stats, h->mp2_stats.p, sizeof(int32_t) * 4 * B, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

int dabphy_mp2_frames_ensemble(dabphy_handle* h, uint32_t ensemble, uint32_t subch_index, dabphy_mp2_event* events, int32_t cap,
                               int32_t* n_events, int32_t* frame_errors, int32_t* first_unverified)
{
    DeviceBind dev_(h);
    static_assert(sizeof(dabphy_mp2_event) == sizeof(Mp2Event), "event layouts must match");
    if (!h || (cap > 0 && !events) || !n_events || !h->last_frames || !h->last_desc || ensemble >= h->cfg.n_ensembles ||
        subch_index >= h->where[ensemble].size()) return DABPHY_ERR_INVALID;
    const dabphy_handle::PairRef w = h->where[ensemble][subch_index];
    const auto& c = h->classes[w.cls];
    if (c.kind[w.pair] != DABPHY_AUDIO_MP2) { h->err = "the sub-channel is not an MP2 service (dabphy_set_audio_kinds_ensemble)"; return DABPHY_ERR_INVALID; }
    int r;
    if (!h->mp2_done && (r = launch_mp2_pass(h, h->last_frames))) return r;
    const uint32_t F = h->last_frames;
    const int n_cif = (int)(4 * F), ev_cap = mp2_ev_cap(F);
    int32_t n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, c.mp2_n.as<int32_t>() + w.pair, sizeof n, hipMemcpyDeviceToHost, h->stream));
    if ((r = sync(h))) return r;
    *n_events = n;
    const int take = std::min(std::min(n, ev_cap), cap);
    if (take > 0) HIPCHK(h, hipMemcpyAsync(events, c.mp2_ev.as<Mp2Event>() + (size_t)w.pair * ev_cap, take * sizeof(Mp2Event), hipMemcpyDeviceToHost, h->stream));
    if (frame_errors) HIPCHK(h, hipMemcpyAsync(frame_errors, c.mp2_err.as<int32_t>() + (size_t)w.pair * n_cif, n_cif * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (first_unverified) HIPCHK(h, hipMemcpyAsync(first_unverified, c.mp2_fu.as<int32_t>() + w.pair, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

int dabphy_get_mp2_ms(dabphy_handle* h, float* ms)
{
    DeviceBind dev_(h);
    if (!h || !ms) return DABPHY_ERR_INVALID;
    *ms = 0.0f;
    if (!h->mp2_timed) return DABPHY_OK;
    HIPCHK(h, hipEventSynchronize(h->ev_mp2[1]));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev_mp2[0], h->ev_mp2[1]));
    return DABPHY_OK;
}

int dabphy_mp2_check(dabphy_handle* h, const uint8_t* frames, uint32_t n_streams, uint32_t n_frames, uint32_t frame_len,
                     dabphy_mp2_event* events, int32_t cap, int32_t* n_events, int32_t* frame_errors, int32_t* first_unverified)
{
    DeviceBind dev_(h);
    if (!h || !frames || !n_streams || !n_frames || !frame_len || frame_len > 2048 || cap < 0 || (cap && !events) || !n_events ||
        !frame_errors || !first_unverified) return DABPHY_ERR_INVALID;
    const size_t bytes = (size_t)n_streams * n_frames * frame_len, stride = mp2_stride();
    int r;
    if ((r = ensure(h, h->in8, bytes))) return r;
    if ((r = ensure(h, h->mp2_chk_state, stride * n_streams))) return r;
    if ((r = ensure(h, h->mp2_chk_ev, (size_t)n_streams * (cap ? cap : 1) * sizeof(Mp2Event)))) return r;
    if ((r = ensure(h, h->mp2_chk_n, n_streams * sizeof(int32_t)))) return r;
    if ((r = ensure(h, h->mp2_chk_err, (size_t)n_streams * n_frames * sizeof(int32_t)))) return r;
    if ((r = ensure(h, h->mp2_chk_fu, n_streams * sizeof(int32_t)))) return r;
    HIPCHK(h, hipMemcpyAsync(h->in8.p, frames, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->mp2_chk_state.p, 0, stride * n_streams, h->stream));       // fresh parsers
    Mp2Args a{};
    a.out = h->in8.as<uint8_t>(); a.n_cif = (int)n_frames; a.frame_bytes = (int)frame_len;
    a.state = h->mp2_chk_state.as<uint8_t>(); a.state_stride = stride;
    a.events = h->mp2_chk_ev.as<Mp2Event>(); a.ev_cap = cap; a.n_events = h->mp2_chk_n.as<int32_t>();
    a.frame_errors = h->mp2_chk_err.as<int32_t>(); a.first_unverified = h->mp2_chk_fu.as<int32_t>();
    launch_mp2(a, (int)n_streams, h->stream);
    if (cap) HIPCHK(h, hipMemcpyAsync(events, a.events, (size_t)n_streams * cap * sizeof(Mp2Event), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(n_events, a.n_events, n_streams * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(frame_errors, a.frame_errors, (size_t)n_streams * n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(first_unverified, a.first_unverified, n_streams * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

} // extern "C"
