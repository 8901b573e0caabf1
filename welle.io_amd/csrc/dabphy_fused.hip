// welle.io_amd/csrc/dabphy_fused.hip -- host side of the fused decode (k_viterbi_fused, k_viterbi.hip): the per-class step tables and the
// launch plan.  No arithmetic of the hot path happens here: the tables restate the depuncturing maps (eep-protection.cpp:32-152,
// uep-protection.cpp:27-239, fic-handler.cpp:158-191) in terms of the kernel's LDS window ring.
#include "dabphy_internal.h"
#include "soft_layout.h"

namespace {

// What every trellis step reads, in terms of a wave's window ring of `rows` rows.  Source byte u of the punctured stream sits in window
// u >> 4 (slot (u >> 4) & 1), column u & 15 -- and, for an MSC class, layout::tdi_row(u & 15) rows below the lane's row base (the time
// de-interleaver, soft_layout.h; the FIC has none).  Returns false when the kernel's window schedule cannot follow the map.
bool step_table(const std::vector<map_t>& m, int nsteps, int n_in, int rows, bool skew, std::vector<MscStep>& st, int& n_windows, int& why)
{
    const int PITCH = MSC_ROW_PITCH, SLOT = rows * MSC_ROW_PITCH, ZERO = 2 * SLOT;
    constexpr int PADDING = 6;                        // the kernel requests descriptors one block of six steps ahead
    st.assign((size_t)nsteps + PADDING, MscStep{0, 0});
    std::vector<int> wlo((size_t)nsteps, -1), whi((size_t)nsteps, -1);
    for (int q = 0; q < nsteps; q++) {
        uint32_t off[4];
        for (int j = 0; j < 4; j++) {
            const int u = map_index(m[4 * q + j]);
            if (u < 0) { off[j] = (uint32_t)ZERO; continue; }
            const int w = u >> 4, col = u & 15;
            off[j] = (uint32_t)((w & 1) * SLOT + (skew ? layout::tdi_row(col) : 0) * PITCH + col);
            if (wlo[q] < 0) wlo[q] = w;
            whi[q] = w;
        }
        st[q].off01 = off[0] | (off[1] << 16); st[q].off23 = off[2] | (off[3] << 16);
    }
    for (int q = nsteps; q < nsteps + PADDING; q++) st[(size_t)q].off01 = st[(size_t)q].off23 = (uint32_t)ZERO | ((uint32_t)ZERO << 16);
    n_windows = (n_in + 15) / 16;
    // lowest window any LATER step reads: when it moves up, the window below it has died and its slot takes the window after the next
    std::vector<int> low_after((size_t)nsteps, n_windows);
    for (int q = nsteps - 2, low = n_windows; q >= 0; q--) { if (wlo[q + 1] >= 0) low = wlo[q + 1]; low_after[q] = low; }
    int seen = 1, prev_low = 0;
    std::vector<int> load_step((size_t)n_windows + 2, -10);
    bool ok = nsteps % 6 == 0; why = ok ? 0 : 8;    // (the kernel walks the trellis in blocks of six steps: true for every 24 * bitrate + 6 and for the FIC's 774)
    for (int q = 0; q < nsteps; q++) {
        if (whi[q] > seen) {
            st[q].off01 |= MSC_FIRST_USE; seen = whi[q];
            // the step BEFORE q waits for the window with s_waitcnt vmcnt(2): its load must be older than two decision stores
            if (q - 1 - load_step[seen] < 2) { ok = false; why |= 1; }
        }
        if (whi[q] >= 0 && whi[q] - wlo[q] > 1) { ok = false; why |= 2; }
        if (low_after[q] > prev_low) {
            if (low_after[q] != prev_low + 1 && low_after[q] < n_windows) { ok = false; why |= 4; }
            prev_low = low_after[q];
            if (prev_low + 1 < n_windows) { st[q].off01 |= MSC_LOAD_NEXT; load_step[prev_low + 1] = q; }
        }
    }
    return ok;
}

}  // namespace

extern "C" {

size_t soft_ens_stride(const dabphy_handle* h)
{
    // [max_frames + 5 frame slots][one frame of zeros]: what the fused decode loads for CIFs that do not exist yet sits behind every
    // ensemble's own slice, inside the reach of a buffer resource based at that slice
    return ((size_t)h->cfg.max_frames + 5 + 1) * SOFT_PER_FRAME;
}

int fused_class_tables(dabphy_handle* h, const dabphy_protection& prot, bool fic, DevBuf (&steps)[FUSED_VARIANTS], int (&n_windows)[FUSED_VARIANTS])
{
    const std::vector<map_t> m = depuncture_map(&prot);
    const int nsteps = prot.nbits + 6, n_in = protection_input_bits(&prot);
    for (int v = 0; v < FUSED_VARIANTS; v++) {
        std::vector<MscStep> st; int nw = 0, why = 0;
        const bool ok = step_table(m, nsteps, n_in, FUSED_ROWS[v], !fic, st, nw, why);
        if (!ok && debug_env("DABPHY_DEBUG")) fprintf(stderr, "dabphy: class nbits %d: no fused decode (window schedule, reason %d)\n", prot.nbits, why);
        n_windows[v] = ok ? nw : 0;                   // (never 0 for the 304 profiles of EN 300 401 and the FIC: tests/test_protection_profiles.py asks dabphy_test_fused_windows; the two-kernel path decodes a class without a schedule)
        int r;
        if ((r = ensure(h, steps[v], st.size() * sizeof(MscStep)))) return r;
        HIPCHK(h, hipMemcpy(steps[v].p, st.data(), st.size() * sizeof(MscStep), hipMemcpyHostToDevice));
    }
    return DABPHY_OK;
}

// The window schedules alone, on the host: what fused_class_tables would record for the class (0 = none for that row count)
int dabphy_test_fused_windows(const dabphy_protection* prot, int32_t n_windows[FUSED_VARIANTS])
{
    if (!prot || !n_windows || !protection_valid(prot) || prot->nbits > PRBS_MAX_BITS) return DABPHY_ERR_INVALID;
    dabphy_protection pf; protection_fic(&pf);
    const bool fic = !memcmp(prot, &pf, sizeof pf);           // (the FIC's rows are not skewed by a time de-interleaver)
    const std::vector<map_t> m = depuncture_map(prot);
    for (int v = 0; v < FUSED_VARIANTS; v++) {
        std::vector<MscStep> st; int nw = 0, why = 0;
        n_windows[v] = step_table(m, prot->nbits + 6, protection_input_bits(prot), FUSED_ROWS[v], !fic, st, nw, why) ? nw : 0;
    }
    return DABPHY_OK;
}

} // extern "C"

namespace {
// ---- The steps of fused_plan, in its order.  First the state-parallel kernels' conditions, stated once for the batch plan and the
// one-class launches.  What the kernels themselves can take: code words in blocks of six steps (true for every 24 * bitrate + 6 and
// the FIC's 774), no longer than their largest LDS build ...
bool sp_kernel_takes(int nsteps) { return nsteps % 6 == 0 && nsteps <= SP_MAXSTEPS[SP_VARIANTS - 1]; }
// ... and what the configuration asks for at n_cw code words: dabphy_config.decode_shape 1 never, 2 / 3 always, 0 up to the code word limit (0: never)
bool sp_wanted(const dabphy_handle* h, uint64_t n_cw) { return h->fused_msc && h->cfg.decode_shape != 1 && (h->cfg.decode_shape >= 2 || (h->sp_max_codewords > 0 && n_cw <= h->sp_max_codewords)); }
// One planning run: what the steps hand on to each other (dabphy_handle::FusedPlan stays as it was until the uploads: a step may fail)
struct Draft {
    uint32_t F = 0; bool want_fic = false; int v = 0;                         // batch depth, the FIC is wanted in the launch, row-count build
    uint64_t total_cw = 0; bool use_sp = false;                               // choose_shape
    std::vector<FusedClass> cls; std::vector<int> idx; bool fic_in = false; size_t max_steps = 0;   // admit_classes (idx: the handle's class of every MSC entry)
    std::vector<uint32_t> work, item_off; uint64_t item_rows = 0;             // build_work_list (item_rows: decision rows -- [64 lanes] cells -- of all groups together)
    bool sp_two = false, tb_split = false, dec_by_item = false; int n_slots = 0; size_t slot_cells = 0, dec_cells = 0;   // lay_out_scratch
};

// A small batch -- fewer code words than the device has lanes to give them -- is decoded STATE-PARALLEL: one wavefront per code word
// (k_viterbi_sp.hip), every class and the FIC, whatever their window schedules and spans (it addresses with 64-bit pointers).
void choose_shape(const dabphy_handle* h, Draft& D)
{
    const bool fic = D.want_fic && h->fused_fic;
    D.total_cw = (uint64_t)h->cfg.n_ensembles * D.F * 4 * (fic ? 1 : 0);
    size_t longest = fic ? 774 : 0; bool takes = true;
    for (auto& c : h->classes) { D.total_cw += (uint64_t)4 * D.F * c.pairs.size(); longest = std::max(longest, (size_t)c.prot.nbits + 6); takes = takes && sp_kernel_takes(c.prot.nbits + 6); }
    // ... and its decision scratch is sized per code word from the LONGEST code word of the launch (decode_work.h: a 256-byte history row
    // per 30 steps): one 384 kbit/s class among small ones makes that 79 KB per code word, 3.2 GB at the code word limit.  The automatic
    // choice therefore also asks for the scratch to stay below a GiB (the lane-per-code-word kernel sizes its scratch per group: dec_by_item)
    const bool scratch_below_a_gib = D.total_cw * (uint64_t)hist_cells(longest, false) * sizeof(uint2) <= ((uint64_t)1 << 30);
    D.use_sp = takes && sp_wanted(h, D.total_cw) && (h->cfg.decode_shape >= 2 || scratch_below_a_gib);
}
// A wave's sources are addressed with 32-bit offsets from the ring slice of its first ensemble.  Its code words span at most
// nseg consecutive (ensemble, sub-channel) pairs of the class's table (64 + 15 nseg <= rows) -- from the first pair's ensemble to the
// last one's, however many ensembles without a sub-channel of this class lie between; the FIC's 64 code words = 16 frames,
// ceil(16 / F) + 1 ensembles.  A class whose span leaves the 4 GiB, or without a window schedule, takes the two-kernel path (64-bit addresses).
void admit_classes(const dabphy_handle* h, Draft& D)
{
    const int nseg = (FUSED_ROWS[D.v] - 64) / 15, F = (int)D.F;
    auto reach_ok = [&](int n_ens_spanned) { return (uint64_t)n_ens_spanned * soft_ens_stride(h) <= 0xffffffffull; };
    auto ens_span = [&](const std::vector<MscPair>& pr) {
        int span = 1;
        for (size_t p = 0; p < pr.size(); p++) span = std::max(span, pr[std::min(pr.size() - 1, p + (size_t)nseg - 1)].ens - pr[p].ens + 1);
        return span;
    };
    for (size_t i = 0; i < h->classes.size(); i++) {
        const auto& c = h->classes[i];
        if (h->fused_msc && (D.use_sp || (c.n_windows[D.v] > 0 && reach_ok(ens_span(c.pairs))))) { D.cls.push_back(msc_fused_class(c, D.F, D.v)); D.idx.push_back((int)i); }
    }
    D.fic_in = D.want_fic && h->fused_fic && (D.use_sp || (h->fic_windows[D.v] > 0 && reach_ok((16 + F - 1) / F + 1)));
    if (D.fic_in) D.cls.push_back(fic_fused_class(h, h->s_fib.as<uint8_t>(), (int)(h->cfg.n_ensembles * D.F * 4), D.v));
    for (const FusedClass& fc : D.cls) D.max_steps = std::max(D.max_steps, (size_t)fc.nsteps);
}
// The work list, longest code words first: the waves that pull the long groups start them while every slot is still busy, the short
// ones fill the end.  Beside every item the first of its decision rows, should the scratch go by group (lay_out_scratch).
int build_work_list(dabphy_handle* h, Draft& D)
{
    if (D.cls.size() > WORK_MAX_CLASSES) { h->err = "more than 255 protection classes"; return DABPHY_ERR_INVALID; }
    struct Item { int nsteps, ci, n_groups; }; std::vector<Item> items;
    for (size_t ci = 0; ci < D.cls.size(); ci++) items.push_back({D.cls[ci].nsteps, (int)ci, (D.cls[ci].n_cw + 63) / 64});
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.nsteps > b.nsteps; });
    for (const Item& it : items) {
        if (it.n_groups > (int)WORK_MAX_GROUPS) { h->err = "class too large for the fused decode's work list"; return DABPHY_ERR_INVALID; }
        for (int g = 0; g < it.n_groups; g++) { D.work.push_back(work_item((uint32_t)it.ci, (uint32_t)g)); D.item_off.push_back((uint32_t)D.item_rows); D.item_rows += (uint64_t)it.nsteps; }
    }
    return DABPHY_OK;
}
// Decision scratch.  State-parallel: one work-group per code word slot -- or pair of slots -- of every listed group, each with the
// history rows of the launch's longest code word (decode_work.h).  Lane per code word: one region per WORK-GROUP sized for the longest
// code word of the launch (reused by every group the wave pulls: the headline's shape) -- unless a few very long code words ride among
// many short ones (one 384 kbit/s service in a multiplex of small ones: 9222 steps x 5120 waves = 24 GB): then one region per GROUP, each
// of its own length.  (The traceback as a pass of its own reads a group's decisions after its wave has gone on to the next: per group.)
void lay_out_scratch(const dabphy_handle* h, Draft& D)
{
    const int slots = fused_wave_slots(D.v);
    D.sp_two = D.use_sp && sp_two_for(h, D.total_cw);
    D.n_slots = D.use_sp ? (int)D.work.size() * (D.sp_two ? 32 : 64) : (int)std::min<size_t>(D.work.size(), (size_t)slots);
    D.slot_cells = D.use_sp ? hist_cells(D.max_steps, D.sp_two) : D.max_steps * 64;
    D.tb_split = h->tb_split && !D.use_sp && D.item_rows < 0xffffffffull && !D.work.empty();
    D.dec_by_item = !D.use_sp && (D.tb_split || debug_env("DABPHY_FORCE_DEC_BY_ITEM") || D.item_rows < (uint64_t)D.n_slots * D.max_steps) && D.item_rows < 0xffffffffull;
    D.dec_cells = D.dec_by_item ? (size_t)D.item_rows * 64 : (size_t)D.n_slots * D.slot_cells;
}
// Every buffer the launch names (nothing for an empty work list); the split traceback's flags, stream and events with the first such plan
int reserve_buffers(dabphy_handle* h, const Draft& D)
{
    int r;
    if (D.work.empty()) return DABPHY_OK;
    if ((r = ensure(h, h->vdec, D.dec_cells * sizeof(uint2))) || (D.dec_by_item && (r = ensure(h, h->fused_dec_off, D.item_off.size() * sizeof(uint32_t))))) return r;
    if (D.tb_split && (r = ensure(h, h->fused_done, (D.work.size() + 2) * sizeof(uint32_t)))) return r;
    if (D.tb_split && !h->tb_stream && ((r = new_stream(h, &h->tb_stream)) || (r = new_event(h, &h->ev_tb_fork)) || (r = new_event(h, &h->ev_tb_join)))) return r;
    if ((r = ensure(h, h->fused_cls, D.cls.size() * sizeof(FusedClass))) || (r = ensure(h, h->fused_work, D.work.size() * sizeof(uint32_t)))) return r;
    return h->d_fused_next ? DABPHY_OK : device_block(h, &h->d_fused_next, 1);
}
// The class table, and the work list with its decision offsets, go up on the handle's stream -- in order with the launches that read
// them -- when their contents changed or any buffer moved (buf_gen); the stream is waited for once, and only when an earlier plan's
// upload can still be reading the host vectors (upload_kept).  It is idle here except inside a call that plans twice.
int upload_changed(dabphy_handle* h, const Draft& D)
{
    auto& P = h->fplan;
    const bool in_place = P.valid && P.buf_gen == h->buf_gen;
    const bool same_cls = in_place && table_holds(P.host_cls, D.cls);
    const bool same_work = in_place && table_holds(P.host_work, D.work) && P.dec_by_item == D.dec_by_item;
    if (P.valid && (!same_cls || !same_work)) HIPCHK(h, hipStreamSynchronize(h->stream));
    int r = same_cls ? 0 : upload_kept(h, h->fused_cls, P.host_cls, D.cls);
    if (!r && !same_work) r = upload_kept(h, h->fused_work, P.host_work, D.work);
    if (!r && !same_work && D.dec_by_item) r = upload_kept(h, h->fused_dec_off, P.host_dec_off, D.item_off);
    return r;
}
// The plan as dabphy_process launches it (launch_plan) and as dabphy_time_fused_msc runs it again: what was decided, the argument block
void keep_plan(dabphy_handle* h, const Draft& D)
{
    auto& P = h->fplan;
    if (debug_env("DABPHY_DEBUG")) fprintf(stderr, "dabphy: decode plan for %u frames per call: %s, %zu of %zu classes%s, %zu groups, %d work-groups, decision scratch %s\n", D.F, D.use_sp ? (D.sp_two ? "state-parallel, two code words per wavefront" : "state-parallel") : "lane-per-code-word", D.idx.size(), h->classes.size(), D.fic_in ? " + FIC" : "", D.work.size(), D.n_slots, D.dec_by_item ? "per group" : "per work-group");
    P.valid = true; P.F = D.F; P.want_fic = D.want_fic; P.fic_in = D.fic_in; P.variant = D.v; P.n_slots = D.n_slots; P.class_idx = D.idx; P.buf_gen = h->buf_gen;
    P.use_sp = D.use_sp; P.sp_variant = sp_variant_for((int)D.max_steps); P.sp_two = D.sp_two; P.dec_by_item = D.dec_by_item; P.tb_split = h->tb_split;
    FusedArgs& a = P.args; a = FusedArgs{};            // (desc stays null: set per batch, the descriptor buffers rotate)
    a.soft = h->s_soft.as<int8_t>(); a.ens_stride = soft_ens_stride(h); a.soft_ring = (int)h->cfg.max_frames + 5; a.n_ens = (int)h->cfg.n_ensembles; a.n_frames = (int)D.F;
    a.cls = h->fused_cls.as<FusedClass>(); a.work = h->fused_work.as<uint32_t>(); a.n_work = (uint32_t)D.work.size(); a.next = h->d_fused_next;
    a.dec = h->vdec.as<uint2>(); a.dec_slot_cells = D.slot_cells; a.prbs_words = h->d_prbs_words;
    a.dec_off = D.dec_by_item ? h->fused_dec_off.as<uint32_t>() : nullptr;
    if (D.tb_split) { a.done = h->fused_done.as<uint32_t>(); a.next_tb = a.done + D.work.size(); }
    a.sp2_warm = (int)h->sp2_tb_warm; a.sp2_resident = (int)h->sp2_tb_resident;
}
}  // namespace

extern "C" {
// The launch plan of one batch depth: which build of the kernel (how many (ensemble, sub-channel) pairs the 64 code words of a wave can
// span), which classes it decodes, their descriptors and the work list.  Called from dabphy_process's allocation phase (every buffer
// it names exists by then).  Everything is a function of the batch depth, the class set and the buffers' addresses (buf_gen moves
// with the last two): an unchanged plan stays.
int fused_plan(dabphy_handle* h, uint32_t F, bool want_fic)
{
    const auto& P = h->fplan;
    if (P.valid && P.F == F && P.want_fic == want_fic && P.buf_gen == h->buf_gen && P.tb_split == h->tb_split) return DABPHY_OK;
    Draft D; D.F = F; D.want_fic = want_fic; D.v = 4 * (int)F >= FUSED_MIN_CIFS[0] ? 0 : 4 * (int)F >= FUSED_MIN_CIFS[1] ? 1 : 2; int r;
    choose_shape(h, D);
    admit_classes(h, D);
    if ((r = build_work_list(h, D))) return r;
    lay_out_scratch(h, D);
    if ((r = reserve_buffers(h, D)) || (r = upload_changed(h, D))) return r;
    keep_plan(h, D);
    return DABPHY_OK;
}
// ... and the launch as queued (FusedPlan::args): state-parallel, or lane per code word -- with the split traceback's stream and events
// when the plan publishes its groups' decisions
void launch_plan(const dabphy_handle* h, hipStream_t s)
{
    const auto& P = h->fplan;
    if (P.use_sp) { launch_sp(P.args, P.sp_two, P.sp_variant, s); return; }
    const FusedSplit split{h->tb_no_walkers ? nullptr : h->tb_stream, h->ev_tb_fork, h->ev_tb_join};
    launch_viterbi_fused(P.args, P.variant, P.n_slots, s, P.args.done ? &split : nullptr);
}
// Whether a stand-alone class of n_cw code words (a seam's call, the replay's one-frame FIC) is decoded state-parallel: the same rule
// as for a batch, within what the one-class launch's work list holds (beyond it the two-kernel path decodes the class)
bool sp_single_ok(const dabphy_handle* h, uint64_t n_cw, int nsteps)
{
    return sp_kernel_takes(nsteps) && n_cw <= (uint64_t)SP_SINGLE_MAX_GROUPS * 64 && sp_wanted(h, n_cw);
}

// One class through k_viterbi_sp on stream st: descriptor and work list go up through a small page-locked staging area (the copies are
// ordered with the launch by the stream; the caller does not reuse the staging before it has synchronised or queued its last launch of
// this class), decision scratch = the handle's (the stream orders it with every other user).  `a` carries what the class kind reads
// (soft / desc / strides, or lin_in / lin_stride); cls, work, dec are filled in here and returned in `a` for further launches.
// every buffer such a launch needs, so that a caller in the middle of a submission (the replay inside dabphy_process) allocates nothing
int sp_single_reserve(dabphy_handle* h, uint64_t n_cw, int nsteps)
{
    const uint64_t n_groups = (n_cw + 63) / 64;
    int r;
    if (n_groups > (uint64_t)SP_SINGLE_MAX_GROUPS) { h->err = "one-class state-parallel launch: too many groups"; return DABPHY_ERR_INVALID; }
    if (!h->h_sp1 && (r = pinned_alloc(h, sizeof(FusedClass) + SP_SINGLE_MAX_GROUPS * sizeof(uint32_t), &h->h_sp1))) return r;
    if ((r = ensure(h, h->sp1_cls, sizeof(FusedClass)))) return r;
    if ((r = ensure(h, h->sp1_work, SP_SINGLE_MAX_GROUPS * sizeof(uint32_t)))) return r;
    return ensure(h, h->vdec, (size_t)n_groups * 64 * hist_cells((size_t)nsteps, false) * sizeof(uint2));
}
int sp_single_prepare(dabphy_handle* h, const FusedClass& fc, FusedArgs& a, hipStream_t st)
{
    const uint32_t n_groups = (uint32_t)((fc.n_cw + 63) / 64);
    int r;
    if ((r = sp_single_reserve(h, (uint64_t)fc.n_cw, fc.nsteps))) return r;
    h->sp1_two = sp_two_for(h, (uint64_t)fc.n_cw);
    FusedClass* hc = reinterpret_cast<FusedClass*>(h->h_sp1);
    uint32_t* hw = reinterpret_cast<uint32_t*>(hc + 1);
    *hc = fc;
    for (uint32_t g = 0; g < n_groups; g++) hw[g] = work_item(0, g);
    HIPCHK(h, hipMemcpyAsync(h->sp1_cls.p, hc, sizeof(FusedClass), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->sp1_work.p, hw, n_groups * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    a.cls = h->sp1_cls.as<FusedClass>(); a.work = h->sp1_work.as<uint32_t>(); a.n_work = n_groups; a.next = nullptr;
    a.dec = h->vdec.as<uint2>(); a.dec_slot_cells = hist_cells((size_t)fc.nsteps, h->sp1_two); a.prbs_words = h->d_prbs_words;
    a.sp2_warm = (int)h->sp2_tb_warm; a.sp2_resident = (int)h->sp2_tb_resident;
    return DABPHY_OK;
}
// The FIC of one class (the replay's one frame at a time, the dabphy_fic_decode seam): state-parallel when sp_single_ok says so -- the
// class goes up once, here -- or through k_fic_gather + k_viterbi.  g names the soft bits and the class; launches take the frame selector.
int fic_one_prepare(dabphy_handle* h, FicOneClass& o, const FicGatherArgs& g, hipStream_t st)
{
    o.g = g; o.v = vit_args(h, g.c); o.spa = FusedArgs{}; o.sp = sp_single_ok(h, (uint64_t)g.c.n_cw, g.c.nsteps);
    if (!o.sp) return DABPHY_OK;
    o.spa.soft = g.soft; o.spa.ens_stride = g.soft_ens_stride ? g.soft_ens_stride : (size_t)g.soft_ring * g.frame_stride; o.spa.soft_ring = g.soft_ring;
    o.spa.n_ens = g.n_ens; o.spa.n_frames = g.n_frames; o.spa.desc = g.desc; o.spa.fic_frame_stride = g.frame_stride;
    return sp_single_prepare(h, fic_fused_class(h, g.c.out, g.c.n_cw, -1), o.spa, st);
}
void fic_one_launch(const dabphy_handle* h, FicOneClass& o, int frame_sel, hipStream_t st)
{
    o.spa.fic_frame_sel = o.g.frame_sel = frame_sel;
    if (o.sp) launch_sp(o.spa, h->sp1_two, sp_variant_for(o.g.c.nsteps), st);
    else { launch_fic_gather(o.g, st); launch_viterbi(o.v, st); }
}
// Two code words per wavefront (k_viterbi_sp2: half the vector instructions per code word) pays once the code words outnumber the SIMDs
// a few times over; below that the launch runs at the latency of ONE wave, and a wave that gathers and walks back two code words takes
// longer than one that does it for one (profiles/r05_viterbi_sp2.txt).  decode_shape 2 / 3 force either kernel.
bool sp_two_for(const dabphy_handle* h, uint64_t n_cw)
{
    if (h->cfg.decode_shape == 3) return false;
    if (h->cfg.decode_shape == 2) return true;
    return n_cw > h->sp2_min_codewords;
}
void launch_sp(const FusedArgs& a, bool two, int lds_variant, hipStream_t s)
{
    if (two) launch_viterbi_sp2(a, lds_variant < SP2_VARIANTS ? lds_variant : SP2_VARIANTS - 1, s); else launch_viterbi_sp(a, lds_variant, s);
}
int sp_variant_for(int nsteps)
{
    int v = 0;
    while (v + 1 < SP_VARIANTS && SP_MAXSTEPS[v] < nsteps) v++;
    return v;
}

} // extern "C"
