// welle.io_amd/csrc/dabphy_chanber.hip -- the channel BER pass (include/dabphy.h: dabphy_set_channel_ber; k_chanber.hip): its tables and
// buffers, the launch behind a batch's final decode, the getters and the stateless entry dabphy_channel_ber.
//
// Records.  One (errors, compared) pair per code word in ONE buffer: the FIC first -- code word (b F + f) 4 + q at record (b F + f) 4 + q --,
// then every protection class in the handle's order, code word pair * 4F + r of class c at first[1 + c] + pair * 4F + r (the code word
// orders of soft_layout.h).  Every totals slot is therefore 4F consecutive records: the FIC of ensemble b from record 4 F b on, list
// position i of ensemble b from its pair's row 0 on.
//
// Order.  The pass is queued on the main stream behind finish_pass (dabphy_process.hip): behind the decoders of every class, the FIC's
// decode wherever it ran, and -- in exact batch mode -- once more behind the replay, so the counts belong to the bytes the getters
// return.  dabphy_process waits for the main stream before it returns, and the next call's demod kernel (the only writer of the
// soft-bit ring) is queued on that stream: on every schedule, with the synchroniser ahead or early, the ring slots the pass reads are
// overwritten only after it.  The deferred superframe filter runs beside it on the auxiliary stream; both only read the class outputs.
#include "dabphy_internal.h"

namespace {
using ChanBer = dabphy_handle::ChanBer;

uint32_t longest_list(const dabphy_handle* h)
{
    size_t n = 0;
    for (const auto& l : h->subch_e) n = std::max(n, l.size());
    return (uint32_t)n;
}

void add_groups(std::vector<uint32_t>& work, uint32_t ci, int64_t n_cw) { for (int64_t g = 0; g < (n_cw + 63) / 64; g++) work.push_back(work_item(ci, (uint32_t)g)); }
}

extern "C" {

int chanber_reserve(dabphy_handle* h, uint32_t F)
{
    ChanBer& c = h->ber;
    if (!c.on) return DABPHY_OK;
    const uint32_t B = h->cfg.n_ensembles, R = 4 * F;
    if (h->classes.size() + 1 > WORK_MAX_CLASSES) { h->err = "more than 254 protection classes with the channel BER pass"; return DABPHY_ERR_INVALID; }
    std::vector<FusedClass> cls; std::vector<uint32_t> work, first, slots;
    uint64_t at = 0;
    cls.push_back(fic_fused_class(h, h->s_fib.as<uint8_t>(), (int)(B * R), -1));
    first.push_back(0); add_groups(work, 0, (int64_t)B * R); at += (uint64_t)B * R;
    for (const auto& mc : h->classes) {
        const FusedClass fc = msc_fused_class(mc, F, -1);                 // (the pass gathers by the map: no step table)
        first.push_back((uint32_t)at); add_groups(work, (uint32_t)cls.size(), fc.n_cw); at += (uint64_t)fc.n_cw;
        cls.push_back(fc);
    }
    if (at >= 0xffffffffull) { h->err = "channel BER pass: too many code words in a batch"; return DABPHY_ERR_INVALID; }
    const uint32_t row_len = 1 + longest_list(h);
    slots.assign((size_t)B * row_len, 0xffffffffu);
    for (uint32_t b = 0; b < B; b++) {
        slots[(size_t)b * row_len] = b * R;
        for (size_t i = 0; i < h->where[b].size(); i++) { const auto w = h->where[b][i]; slots[(size_t)b * row_len + 1 + i] = first[1 + w.cls] + (uint32_t)w.pair * R; }
    }
    int r;
    if ((r = ensure(h, c.counts, std::max<uint64_t>(at, 1) * sizeof(uint2)))) return r;
    if ((r = ensure(h, c.totals, (size_t)B * row_len * 2 * sizeof(uint64_t)))) return r;
    if ((r = upload_if_changed(h, c.cls, c.host_cls, cls)) || (r = upload_if_changed(h, c.work, c.host_work, work)) ||
        (r = upload_if_changed(h, c.first, c.host_first, first)) || (r = upload_if_changed(h, c.slots, c.host_slots, slots))) return r;
    if (c.F != F || c.row_len != row_len) c.counted = false;
    c.F = F; c.row_len = row_len;
    if (h->profiling && !c.ev[0] && ((r = new_event(h, &c.ev[0], true)) || (r = new_event(h, &c.ev[1], true)))) return r;   // (dabphy_get_chanber_ms)
    return DABPHY_OK;
}

int chanber_pass(dabphy_handle* h, const FrameDesc* desc, uint32_t F)
{
    ChanBer& c = h->ber;
    if (!c.on) return DABPHY_OK;
    BerArgs a{};
    a.f.soft = h->s_soft.as<int8_t>(); a.f.ens_stride = soft_ens_stride(h); a.f.soft_ring = (int)h->cfg.max_frames + 5;
    a.f.n_ens = (int)h->cfg.n_ensembles; a.f.n_frames = (int)F; a.f.desc = desc;
    a.f.cls = c.cls.as<FusedClass>(); a.f.work = c.work.as<uint32_t>(); a.f.n_work = (uint32_t)c.host_work.size(); a.f.prbs_words = h->d_prbs_words;
    a.first = c.first.as<uint32_t>(); a.out = c.counts.as<uint2>();
    BerTotalsArgs t{}; t.counts = a.out; t.slots = c.slots.as<uint32_t>(); t.n = 4 * F; t.totals = c.totals.as<uint64_t>();
    const bool timed = h->profiling && c.ev[0] && c.ev[1];
    if (timed) HIPCHK(h, hipEventRecord(c.ev[0], h->stream));
    launch_chanber(a, h->stream);
    launch_chanber_totals(t, (int)c.host_slots.size(), h->stream);
    if (timed) HIPCHK(h, hipEventRecord(c.ev[1], h->stream));
    c.timed = timed; c.counted = true;
    return DABPHY_OK;
}

void chanber_clear(dabphy_handle* h) { h->ber.counted = false; h->ber.timed = false; }

int dabphy_set_channel_ber(dabphy_handle* h, int32_t on)
{
    DeviceBind dev_(h);
    if (!h || on < 0 || on > 1) return DABPHY_ERR_INVALID;
    ChanBer& c = h->ber;
    if ((on != 0) == c.on) return DABPHY_OK;
    chanber_clear(h);
    c.on = on != 0;
    if (c.on) {
        // what can be sized now (the lists as applied, the handle's batch depth); dabphy_process reserves for the lists and depth it meets
        if (!h->where.empty() && !h->subch_dirty && h->s_fib.p) return chanber_reserve(h, h->cfg.max_frames);
        return DABPHY_OK;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (DevBuf* b : {&c.cls, &c.work, &c.first, &c.slots, &c.counts, &c.totals}) b->release();
    c.host_cls.clear(); c.host_work.clear(); c.host_first.clear(); c.host_slots.clear(); c.F = c.row_len = 0;
    return DABPHY_OK;
}

static int ber_ready(dabphy_handle* h)
{
    if (!h->ber.on) { h->err = "the channel BER pass is off (dabphy_set_channel_ber)"; return DABPHY_ERR_STATE; }
    if (!h->ber.counted || !h->last_frames || h->last_frames != h->ber.F) { h->err = "no batch has been counted since the channel BER pass was switched on, the last reset or the last change of a sub-channel list"; return DABPHY_ERR_STATE; }
    return DABPHY_OK;
}

int dabphy_get_channel_ber_fic(dabphy_handle* h, dabphy_ber_count* out)
{
    DeviceBind dev_(h);
    static_assert(sizeof(dabphy_ber_count) == sizeof(uint2), "count records must match");
    if (!h || !out) return DABPHY_ERR_INVALID;
    if (int r = ber_ready(h)) return r;
    HIPCHK(h, hipMemcpyAsync(out, h->ber.counts.p, (size_t)h->cfg.n_ensembles * h->ber.F * 4 * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}

int dabphy_get_channel_ber_ensemble(dabphy_handle* h, uint32_t ensemble, uint32_t subch_index, dabphy_ber_count* out, size_t out_capacity,
                                    int32_t* first_valid, int32_t* n_rows)
{
    DeviceBind dev_(h);
    if (!h || !out) return DABPHY_ERR_INVALID;
    if (int r = ber_ready(h)) return r;
    if (ensemble >= h->cfg.n_ensembles || subch_index >= h->where[ensemble].size()) return DABPHY_ERR_INVALID;
    const uint32_t R = 4 * h->ber.F;
    if (out_capacity < R) { h->err = "dabphy_get_channel_ber_ensemble: output buffer too small"; return DABPHY_ERR_INVALID; }
    const dabphy_handle::PairRef w = h->where[ensemble][subch_index];
    HIPCHK(h, hipMemcpyAsync(out, h->ber.counts.as<uint2>() + h->ber.host_first[1 + w.cls] + (size_t)w.pair * R, R * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    msc_rows_info(h, ensemble, w, first_valid, n_rows);
    return sync(h);
}

int dabphy_get_channel_ber_totals(dabphy_handle* h, uint64_t* errors, uint64_t* compared, uint32_t* row_len)
{
    DeviceBind dev_(h);
    if (!h || (!errors != !compared) || (!errors && !row_len)) return DABPHY_ERR_INVALID;
    if (int r = ber_ready(h)) return r;
    if (row_len) *row_len = h->ber.row_len;
    if (!errors) return DABPHY_OK;                     // (the row length alone: what the arrays must hold)
    const size_t n = (size_t)h->cfg.n_ensembles * h->ber.row_len;
    std::vector<uint64_t> t(2 * n);
    HIPCHK(h, hipMemcpyAsync(t.data(), h->ber.totals.p, t.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (int r = sync(h)) return r;
    for (size_t i = 0; i < n; i++) { errors[i] = t[2 * i]; compared[i] = t[2 * i + 1]; }
    return DABPHY_OK;
}

int dabphy_get_chanber_ms(dabphy_handle* h, float* ms)
{
    DeviceBind dev_(h);
    if (!h || !ms) return DABPHY_ERR_INVALID;
    *ms = 0.0f;
    if (!h->ber.timed) return DABPHY_OK;
    HIPCHK(h, hipEventSynchronize(h->ber.ev[1]));
    HIPCHK(h, hipEventElapsedTime(ms, h->ber.ev[0], h->ber.ev[1]));
    return DABPHY_OK;
}

int dabphy_channel_ber(dabphy_handle* h, const dabphy_protection* prot, const int8_t* in, const uint8_t* decoded, uint32_t n_codewords, dabphy_ber_count* out)
{
    DeviceBind dev_(h);
    if (!h || !prot || !in || !decoded || !out || n_codewords == 0 || !protection_valid(prot) || prot->nbits > PRBS_MAX_BITS) return DABPHY_ERR_INVALID;
    const uint32_t n_groups = (n_codewords + 63) / 64;
    if (n_groups > WORK_MAX_GROUPS) { h->err = "dabphy_channel_ber: too many code words"; return DABPHY_ERR_INVALID; }
    const std::vector<map_t> m = depuncture_map(prot);
    const size_t n_in = (size_t)protection_input_bits(prot), nbytes = (size_t)prot->nbits / 8;
    // the table: the class, the first record of class 0, the work list
    std::vector<uint32_t> tab(sizeof(FusedClass) / 4 + 4 + n_groups, 0u);
    int r;
    if ((r = ensure(h, h->map, m.size() * sizeof(map_t))) || (r = ensure(h, h->in8, n_in * n_codewords)) || (r = ensure(h, h->vout, nbytes * n_codewords)) ||
        (r = ensure(h, h->ber_lin_tab, tab.size() * 4)) || (r = ensure(h, h->ber_lin_out, (size_t)n_codewords * sizeof(uint2)))) return r;
    FusedClass fc{};
    fc.map = h->map.as<map_t>(); fc.out = h->vout.as<uint8_t>(); fc.nbits = prot->nbits; fc.nsteps = prot->nbits + 6; fc.n_cw = (int32_t)n_codewords; fc.n_pairs = 1;
    fc.kind = 2; fc.dedisperse = 1;
    memcpy(tab.data(), &fc, sizeof fc);
    for (uint32_t g = 0; g < n_groups; g++) tab[sizeof(FusedClass) / 4 + 4 + g] = work_item(0, g);
    HIPCHK(h, hipMemcpyAsync(h->map.p, m.data(), m.size() * sizeof(map_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->in8.p, in, n_in * n_codewords, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->vout.p, decoded, nbytes * n_codewords, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->ber_lin_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
    BerArgs a{};
    a.f.n_ens = 1; a.f.n_frames = 1; a.f.lin_in = h->in8.as<int8_t>(); a.f.lin_stride = n_in; a.f.prbs_words = h->d_prbs_words;
    a.f.cls = h->ber_lin_tab.as<FusedClass>(); a.first = h->ber_lin_tab.as<uint32_t>() + sizeof(FusedClass) / 4; a.f.work = a.first + 4; a.f.n_work = n_groups;
    a.out = h->ber_lin_out.as<uint2>();
    launch_chanber(a, h->stream);
    HIPCHK(h, hipMemcpyAsync(out, a.out, (size_t)n_codewords * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    return sync(h);                                    // (m and tab live until here)
}

} // extern "C"
