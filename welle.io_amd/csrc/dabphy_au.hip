// welle.io_amd/csrc/dabphy_au.hip -- the bulk access-unit drain (include/dabphy.h: dabphy_set_au_drain): the pack pass queued behind every
// all-sub-channel filter pass (k_au.hip), its tables, and the copy of a pass's access units to the host.  Every access to h->au is here
// (dabphy_reset drops a pass that was not drained).
#include "dabphy_internal.h"

extern "C" {

namespace {
using Au = dabphy_handle::AuDrain;
static_assert(sizeof(dabphy_au_desc) == sizeof(AuRec) && sizeof(dabphy_au_desc) == 24 && sizeof(dabphy_au_service) == 48, "access-unit record layouts");
constexpr size_t PIECE = (size_t)4 << 20;            // (pieces of a few MB, as the MSC drain's: small transfers of the next batch share the copy engine)

// What one (ensemble, sub-channel) pair of `s` code words per superframe can store in a batch of n_slots superframes: per superframe at
// most 110 s payload bytes in at most 6 access units, each with at most 11 bytes of LOAS header and padding and one length byte per
// 255 bytes of payload (or part of them); whole 16-byte pieces
size_t au_reserve(int s, int n_slots) { const size_t sf = (size_t)110 * s; return ((size_t)n_slots * (sf + 6 * 11 + sf / 255 + 6) + 15) & ~(size_t)15; }

int events_ready(dabphy_handle* h)
{
    Au& a = h->au; int r;
    if (!a.ev_packed && ((r = new_event(h, &a.ev_packed)) || (r = new_event(h, &a.ev_done)) || (r = new_event(h, &a.ev_time[0], true)) || (r = new_event(h, &a.ev_time[1], true)))) return r;
    return DABPHY_OK;
}
// (re)allocated blocks start as zeros: the padding of the staging buffer and the unused records cross to the host too
int ensure_zeroed(dabphy_handle* h, DevBuf& b, size_t bytes, hipStream_t st)
{
    const size_t before = b.cap; int r;                    // (ensure only ever grows a block: a new capacity is a new block, whatever its address)
    if ((r = ensure(h, b, bytes))) return r;
    if (b.cap != before) HIPCHK(h, hipMemsetAsync(b.p, 0, b.cap, st));
    return DABPHY_OK;
}
}

int au_drain_wait(dabphy_handle* h)
{
    Au& a = h->au;
    if (!a.inflight) return DABPHY_OK;
    a.inflight = false;
    HIPCHK(h, hipEventSynchronize(a.ev_done));
    for (size_t k = 0; k < a.flight.services.size(); k++) {          // the service records: what the host knew when the pass was queued + what the device counted
        dabphy_au_service s = a.flight.services[k];
        const AuSvc& d = a.h_svc[a.flight.slot[k]];
        s.n_superframes = d.n_superframes; s.n_aus = d.n_aus; s.n_failed = d.n_failed; s.bytes = d.bytes;
        a.out_services[k] = s;
    }
    return DABPHY_OK;
}

int au_pack_pass(dabphy_handle* h, const std::vector<SfSel>& sel, hipStream_t st, uint32_t F)
{
    Au& a = h->au; int r;
    if (!a.format || sel.empty()) return DABPHY_OK;
    const uint32_t B = h->cfg.n_ensembles;
    const int n_cif = (int)(4 * F), n_slots = n_cif / 5 + 1, au_cap = n_slots * 6;
    if ((r = events_ready(h))) return r;
    // layout of the staging buffer: one region per DAB+-rate class, 256-byte aligned, one reservation per pair
    std::vector<size_t> region0(h->classes.size(), 0), reserve(h->classes.size(), 0);
    size_t total = 0;
    for (size_t c = 0; c < h->classes.size(); c++) {
        const auto& cls = h->classes[c];
        if (!cls.dabplus_rate()) continue;
        region0[c] = total; reserve[c] = au_reserve(cls.prot.nbits / 24 / 8, n_slots);
        total += (cls.pairs.size() * reserve[c] + 255) & ~(size_t)255;
    }
    std::vector<int32_t> base(B); uint32_t n_all = 0;
    for (uint32_t b = 0; b < B; b++) { base[b] = (int32_t)n_all; n_all += (uint32_t)h->where[b].size(); }
    if ((r = ensure_zeroed(h, a.stage, total, st)) || (r = ensure_zeroed(h, a.svc, (size_t)n_all * sizeof(AuSvc), st)) ||
        (r = ensure_zeroed(h, a.tab, (size_t)n_all * au_cap * sizeof(AuRec), st)) || (r = ensure(h, a.src, (size_t)n_all * au_cap * sizeof(uint2)))) return r;
    if (a.base.cap < B * sizeof(int32_t) || base != a.base_host) {
        // (the lists change only between passes, behind a flushed pass: nothing in flight reads the old table; a.base_host outlives the copy)
        if ((r = ensure(h, a.base, B * sizeof(int32_t)))) return r;
        a.base_host = base;
        HIPCHK(h, hipMemcpyAsync(a.base.p, a.base_host.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    if (a.inflight) HIPCHK(h, hipStreamWaitEvent(st, a.ev_done, 0));      // the drain in flight reads what this pass overwrites
    if (h->profiling) { hipError_t e = hipEventRecord(a.ev_time[0], st); (void)e; }
    for (const SfSel& e : sel) {
        auto& cls = h->classes[e.cls];
        if (!cls.dabplus_rate() || cls.pairs.empty()) continue;
        AuArgs k{};
        k.events = h->sf_events.as<SfEvent>() + cls.sf_pair0 * n_cif; k.n_events = h->sf_count.as<int32_t>() + cls.sf_pair0; k.n_cif = n_cif;
        k.sf = h->sf_bytes.as<uint8_t>() + cls.sf_bytes0; k.n_slots = n_slots; k.sf_len = 5 * (cls.prot.nbits / 8);
        k.run = e.d_run; k.pairs = cls.pair_tab.as<MscPair>(); k.ens_base = a.base.as<int32_t>(); k.format = a.format;
        k.stage = a.stage.as<uint8_t>(); k.region0 = region0[e.cls]; k.reserve = reserve[e.cls];
        k.svc = a.svc.as<AuSvc>(); k.aus = a.tab.as<AuRec>(); k.au_src = a.src.as<uint2>(); k.au_cap = au_cap;
        launch_au_pack(k, e.d_run ? e.n_run : (int)cls.pairs.size(), st);
    }
    if (h->profiling) { hipError_t e = hipEventRecord(a.ev_time[1], st); (void)e; a.timed = true; }
    HIPCHK(h, hipEventRecord(a.ev_packed, st));
    // what a drain of this pass needs from the host, as it is NOW
    Au::Layout& L = a.last;
    L.services.clear(); L.slot.clear(); L.bytes = total; L.n_positions = n_all; L.au_cap = (uint32_t)au_cap; L.format = a.format;
    for (uint32_t b = 0; b < B; b++)
        for (size_t i = 0; i < h->where[b].size(); i++) {
            const dabphy_handle::PairRef w = h->where[b][i];
            const auto& cls = h->classes[w.cls];
            if (!cls.dabplus_rate() || cls.kind[w.pair] == DABPHY_AUDIO_MP2) continue;
            dabphy_au_service s{};
            s.ensemble = b; s.subch_index = (uint32_t)i; s.subch_id = (uint32_t)cls.subch_id[w.pair];
            s.first_au = (uint32_t)((base[b] + i) * au_cap); s.offset = region0[w.cls] + (uint64_t)w.pair * reserve[w.cls];
            L.services.push_back(s); L.slot.push_back((uint32_t)(base[b] + i));
        }
    a.packed = a.known = true;
    return DABPHY_OK;
}

int dabphy_set_au_drain(dabphy_handle* h, int32_t format)
{
    DeviceBind dev_(h);
    if (!h || format < DABPHY_AU_OFF || format > DABPHY_AU_LOAS) return DABPHY_ERR_INVALID;
    if (format == h->au.format) return DABPHY_OK;
    int r = au_drain_wait(h); if (r) return r;
    h->au.packed = false; h->au.format = format;
    if (format == DABPHY_AU_OFF) h->au.known = false;
    return DABPHY_OK;
}

int dabphy_au_batch_size(dabphy_handle* h, size_t* buf_bytes, uint32_t* n_services, uint32_t* n_aus_capacity)
{
    if (!h) return DABPHY_ERR_INVALID;
    if (!h->au.known) { h->err = "dabphy_au_batch_size: no filter pass has run since the drain was switched on"; return DABPHY_ERR_STATE; }
    const Au::Layout& L = h->au.last;
    if (buf_bytes) *buf_bytes = L.bytes;
    if (n_services) *n_services = (uint32_t)L.services.size();
    if (n_aus_capacity) *n_aus_capacity = L.n_positions * L.au_cap;
    return DABPHY_OK;
}

int dabphy_au_drain_begin(dabphy_handle* h, dabphy_au_service* services, uint32_t services_capacity, dabphy_au_desc* aus, uint32_t aus_capacity, uint8_t* buf, size_t buf_capacity)
{
    DeviceBind dev_(h);
    if (!h || (!services && services_capacity)) return DABPHY_ERR_INVALID;
    Au& a = h->au; int r;
    if (!a.packed) { h->err = "dabphy_au_drain_begin: no filter pass has run with the drain on since the last drain"; return DABPHY_ERR_STATE; }
    const Au::Layout& L = a.last;
    const size_t n_rec = (size_t)L.n_positions * L.au_cap;
    if (L.services.size() > services_capacity || (aus && n_rec > aus_capacity) || L.bytes > buf_capacity || (L.bytes && !buf)) {
        h->err = "dabphy_au_drain_begin: buffer or table too small (dabphy_au_batch_size)"; return DABPHY_ERR_INVALID;
    }
    if ((r = au_drain_wait(h))) return r;                   // one access-unit drain at a time
    if ((r = drain_stream_ready(h))) return r;
    if (a.h_svc_cap < L.n_positions) {                      // (grows with the lists; the outgrown block goes: no drain is in flight here)
        if (a.h_svc) {
            h->pinned.erase(std::remove(h->pinned.begin(), h->pinned.end(), (void*)a.h_svc), h->pinned.end());
            hipError_t e = hipHostFree(a.h_svc); (void)e; a.h_svc = nullptr; a.h_svc_cap = 0;
        }
        if ((r = pinned_alloc(h, (size_t)L.n_positions * sizeof(AuSvc), &a.h_svc))) return r;
        a.h_svc_cap = L.n_positions;
    }
    HIPCHK(h, hipStreamWaitEvent(h->drain_stream, a.ev_packed, 0));
    for (size_t at = 0; at < L.bytes; at += PIECE)
        HIPCHK(h, hipMemcpyAsync(buf + at, a.stage.as<uint8_t>() + at, std::min(PIECE, L.bytes - at), hipMemcpyDeviceToHost, h->drain_stream));
    if (aus) {
        const size_t bytes = n_rec * sizeof(AuRec);
        for (size_t at = 0; at < bytes; at += PIECE)
            HIPCHK(h, hipMemcpyAsync(reinterpret_cast<uint8_t*>(aus) + at, a.tab.as<uint8_t>() + at, std::min(PIECE, bytes - at), hipMemcpyDeviceToHost, h->drain_stream));
    }
    if (L.n_positions) HIPCHK(h, hipMemcpyAsync(a.h_svc, a.svc.p, (size_t)L.n_positions * sizeof(AuSvc), hipMemcpyDeviceToHost, h->drain_stream));
    HIPCHK(h, hipEventRecord(a.ev_done, h->drain_stream));
    a.flight = a.last; a.out_services = services; a.out_aus = aus != nullptr;
    a.packed = false; a.inflight = true;
    return DABPHY_OK;
}

int dabphy_au_drain_wait(dabphy_handle* h, uint32_t* n_services, uint32_t* n_aus)
{
    DeviceBind dev_(h);
    if (!h) return DABPHY_ERR_INVALID;
    int r = au_drain_wait(h); if (r) return r;
    if (n_services) *n_services = (uint32_t)h->au.flight.services.size();
    if (n_aus) *n_aus = h->au.out_aus ? h->au.flight.n_positions * h->au.flight.au_cap : 0;
    return DABPHY_OK;
}

int dabphy_get_au_batch(dabphy_handle* h, dabphy_au_service* services, uint32_t services_capacity, dabphy_au_desc* aus, uint32_t aus_capacity,
                        uint8_t* buf, size_t buf_capacity, uint32_t* n_services, uint32_t* n_aus)
{
    int r = dabphy_au_drain_begin(h, services, services_capacity, aus, aus_capacity, buf, buf_capacity);
    return r ? r : dabphy_au_drain_wait(h, n_services, n_aus);
}

int dabphy_get_au_ms(dabphy_handle* h, float* ms)
{
    DeviceBind dev_(h);
    if (!h || !ms) return DABPHY_ERR_INVALID;
    *ms = 0.0f;
    if (h->au.timed && hipEventSynchronize(h->au.ev_time[1]) == hipSuccess) { float t = 0; if (hipEventElapsedTime(&t, h->au.ev_time[0], h->au.ev_time[1]) == hipSuccess) *ms = t; }
    return DABPHY_OK;
}

int dabphy_test_au_pack(dabphy_handle* h, const uint8_t* sf, const dabphy_sf_event* events, uint32_t n_events, uint32_t n_sf, uint32_t s_per_sf,
                        int32_t format, uint8_t* out, size_t out_capacity, dabphy_au_desc* aus, uint32_t aus_capacity, dabphy_au_service* service)
{
    DeviceBind dev_(h);
    if (!h || !sf || !events || !out || !service || (!aus && aus_capacity) || !n_sf || !s_per_sf || s_per_sf > 48 || (format != DABPHY_AU_RAW && format != DABPHY_AU_LOAS)) return DABPHY_ERR_INVALID;
    const size_t sf_len = (size_t)120 * s_per_sf, cap = (out_capacity + 15) & ~(size_t)15;
    const size_t n_ev = std::max<size_t>(n_events, 1), n_rec = std::max<uint32_t>(aus_capacity, 1);
    // scratch of this call alone (the handle's drain keeps its own buffers): events, count, superframes, the region, the tables
    DevBuf d_ev, d_n, d_sf, d_out, d_svc, d_tab, d_src; int r;
    if ((r = dev_alloc(h, d_ev, n_ev * sizeof(SfEvent))) || (r = dev_alloc(h, d_n, sizeof(int32_t))) || (r = dev_alloc(h, d_sf, sf_len * n_sf)) || (r = dev_alloc(h, d_out, std::max<size_t>(cap, 16))) ||
        (r = dev_alloc(h, d_svc, sizeof(AuSvc))) || (r = dev_alloc(h, d_tab, n_rec * sizeof(AuRec))) || (r = dev_alloc(h, d_src, n_rec * sizeof(uint2)))) return r;
    const int32_t ne = (int32_t)n_events;
    if (n_events) HIPCHK(h, hipMemcpyAsync(d_ev.p, events, n_events * sizeof(SfEvent), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_n.p, &ne, sizeof ne, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_sf.p, sf, sf_len * n_sf, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_out.p, 0, d_out.cap, h->stream));
    HIPCHK(h, hipMemsetAsync(d_tab.p, 0, d_tab.cap, h->stream));
    AuArgs k{};
    k.events = d_ev.as<SfEvent>(); k.n_events = d_n.as<int32_t>(); k.n_cif = (int)n_ev; k.sf = d_sf.as<uint8_t>(); k.n_slots = (int)n_sf; k.sf_len = (int)sf_len;
    k.format = format; k.stage = d_out.as<uint8_t>(); k.region0 = 0; k.reserve = out_capacity;
    k.svc = d_svc.as<AuSvc>(); k.aus = d_tab.as<AuRec>(); k.au_src = d_src.as<uint2>(); k.au_cap = (int)aus_capacity;
    launch_au_pack(k, 1, h->stream);
    AuSvc got{};
    HIPCHK(h, hipMemcpyAsync(out, d_out.p, out_capacity, hipMemcpyDeviceToHost, h->stream));
    if (aus_capacity) HIPCHK(h, hipMemcpyAsync(aus, d_tab.p, (size_t)aus_capacity * sizeof(AuRec), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&got, d_svc.p, sizeof got, hipMemcpyDeviceToHost, h->stream));
    if ((r = sync(h))) return r;
    memset(service, 0, sizeof *service);
    service->n_superframes = got.n_superframes; service->n_aus = got.n_aus; service->n_failed = got.n_failed; service->bytes = got.bytes;
    return DABPHY_OK;
}

} // extern "C"
