// oracle/ref_acquire_harness.cpp -- TEST INFRASTRUCTURE: the reference's own OFDMProcessor::run over a caller's stream, recording what
// its acquisition head does: every window search (where its 2048 samples begin in the stream, whether it found a window, its impulse
// response) and the onSyncChange counts.  Built by oracle/Makefile into _ref/libwelle_ref_acquire.so from the unmodified sources (the
// objects of libwelle_ref.so); a library of its own beside the harness library, like libwelle_ref_prs.so, so that the tap exists
// whatever the age of the harness library and ref_run_io keeps its layout.  Nothing here restates an algorithm: the function builds the
// reference's RadioReceiver over an in-memory input, as the end-to-end tap of ref_harness.cpp does, and listens.
#include <atomic>
#include <chrono>
#include <complex>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "radio-receiver.h"

namespace {

struct Listener : RadioControllerInterface {
    const int64_t* in_pos = nullptr;                                  // the input's read position
    int64_t* att_pos = nullptr; int32_t* att_true = nullptr; float* cir = nullptr; int cap = 0;
    std::atomic<int> n_att{0}, n_sync_true{0}, n_sync_false{0}, n_nul{0}, n_con{0};
    std::atomic<bool> failed{false};
    void onSNR(float) override {}
    void onFrequencyCorrectorChange(int, int) override {}
    void onSyncChange(char s) override { if (s) n_sync_true++; else n_sync_false++; }
    void onSignalPresence(bool) override {}
    void onServiceDetected(uint32_t) override {}
    void onNewEnsemble(uint16_t) override {}
    void onSetEnsembleLabel(DabLabel&) override {}
    void onDateTimeUpdate(const dab_date_time_t&) override {}
    void onFIBDecodeSuccess(bool, const uint8_t*) override {}
    // called on the thread that pulls the samples, right behind the one getSamples(T_u) of the search and before anything else is
    // pulled (ofdm-processor.cpp:337-344): the input's read position is the end of the searched window.  onSyncChange(true) follows
    // on the same thread if the search found a window (:371): the count seen by the NEXT attempt tells
    void onNewImpulseResponse(std::vector<float>&& d) override {
        const int k = n_att++;
        if (k < cap) {
            att_pos[k] = *in_pos - 2048; att_true[k] = n_sync_true.load();
            if (cir && d.size() == 2048) memcpy(cir + 2048 * (size_t)k, d.data(), 2048 * sizeof(float));
        }
    }
    void onConstellationPoints(std::vector<DSPCOMPLEX>&&) override { n_con++; }
    void onNewNullSymbol(std::vector<DSPCOMPLEX>&&) override { n_nul++; }
    void onTIIMeasurement(tii_measurement_t&&) override {}
    void onMessage(message_level_t, const std::string&, const std::string&) override {}
    void onInputFailure() override { failed = true; }
};

// In-memory input with the lock-step gate of ref_harness.cpp: the pulling thread never gets a new frame while the decoder thread
// still owes the previous one (the coarse corrector reads the decoder's FIC ratio, ofdm-processor.cpp:397)
struct MemInput : InputInterface {
    const DSPCOMPLEX* data; int64_t n; int64_t pos = 0; Listener* rec; std::atomic<bool> armed{false};
    MemInput(const float* iq, int64_t n_, Listener* r) : data((const DSPCOMPLEX*)iq), n(n_), rec(r) {}
    void setFrequency(int) override {}
    int getFrequency() const override { return 0; }
    bool is_ok() override { return n - pos >= 2656; }
    bool restart() override { return true; }
    void stop() override {}
    void reset() override {}
    int32_t getSamples(DSPCOMPLEX* b, int32_t size) override {
        int64_t k = size; if (k > n - pos) k = n - pos;
        memcpy(b, data + pos, k * sizeof(DSPCOMPLEX)); pos += k; return (int32_t)k;
    }
    std::vector<DSPCOMPLEX> getSpectrumSamples(int) override { return {}; }
    int32_t getSamplesToRead() override {
        if (!armed) return 0;
        if (rec->n_nul.load() > rec->n_con.load()) return 0;
        int64_t k = n - pos; if (k > 2656) k = 2656; return (int32_t)k;
    }
    float setGain(int) override { return 0; }
    float getGain() const override { return 0; }
    int getGainCount() override { return 0; }
    void setAgc(bool) override {}
    std::string getDescription() override { return "mem"; }
};

} // namespace

// att_pos / att_true / cir (cap entries, cir 2048 floats each, may be NULL): per window search the stream position of its first
// sample, the onSyncChange(true) calls before it, its impulse response.  counts[3] = window searches made (kept or not),
// onSyncChange(true) calls, onSyncChange(false) calls.  Default receiver options (ThresholdBeforePeak, PatternOfZeros).
extern "C" int ref_acquire_run(const float* iq, int64_t n_samples, int64_t* att_pos, int32_t* att_true, float* cir, int32_t cap, int32_t* counts)
{
    Listener rec;
    MemInput in(iq, n_samples, &rec);
    rec.in_pos = &in.pos; rec.att_pos = att_pos; rec.att_true = att_true; rec.cir = cir; rec.cap = (att_pos && att_true) ? cap : 0;
    RadioReceiverOptions rro;
    rro.decodeTII = false;
    {
        RadioReceiver rx(rec, in, rro);
        rx.restart(false);
        in.armed = true;
        while (!rec.failed) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        rx.stop();                       // the pulling thread has ended (it reported the input's failure): every attempt is on record
    }
    counts[0] = rec.n_att; counts[1] = rec.n_sync_true; counts[2] = rec.n_sync_false;
    return 0;
}
