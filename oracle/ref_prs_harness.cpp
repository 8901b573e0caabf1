// oracle/ref_prs_harness.cpp -- TEST INFRASTRUCTURE: the reference's own OFDMProcessor::processPRS (ofdm-processor.cpp:537-616, with
// getMiddle, :618-644) on a caller's 2048 samples.  Built by oracle/Makefile into _ref/libwelle_ref_prs.so from the unmodified sources
// (the objects of libwelle_ref.so); a library of its own beside the harness library, like libwelle_ref_subch.so, so that the tap exists
// whatever the age of the harness library.  Nothing here restates an algorithm: the function builds the reference's RadioReceiver as
// the end-to-end tap of ref_harness.cpp does -- it owns the OFDMProcessor and everything that refers to -- and forwards the call.  The
// receiver is never restarted: no thread is started and nothing is read from the input.
#include <complex>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
// processPRS is a private member.  The reference sources are not edited -- this translation unit only relaxes access control for itself.
#define private public
#define protected public
#include "radio-receiver.h"
#undef private
#undef protected

namespace {

struct NoController : RadioControllerInterface {
    void onSNR(float) override {}
    void onFrequencyCorrectorChange(int, int) override {}
    void onSyncChange(char) override {}
    void onSignalPresence(bool) override {}
    void onServiceDetected(uint32_t) override {}
    void onNewEnsemble(uint16_t) override {}
    void onSetEnsembleLabel(DabLabel&) override {}
    void onDateTimeUpdate(const dab_date_time_t&) override {}
    void onFIBDecodeSuccess(bool, const uint8_t*) override {}
    void onNewImpulseResponse(std::vector<float>&&) override {}
    void onConstellationPoints(std::vector<DSPCOMPLEX>&&) override {}
    void onNewNullSymbol(std::vector<DSPCOMPLEX>&&) override {}
    void onTIIMeasurement(tii_measurement_t&&) override {}
    void onMessage(message_level_t, const std::string&, const std::string&) override {}
    void onInputFailure() override {}
};

struct NoInput : InputInterface {
    void setFrequency(int) override {}
    int getFrequency() const override { return 0; }
    bool is_ok() override { return false; }
    bool restart() override { return true; }
    void stop() override {}
    void reset() override {}
    int32_t getSamples(DSPCOMPLEX*, int32_t) override { return 0; }
    std::vector<DSPCOMPLEX> getSpectrumSamples(int) override { return {}; }
    int32_t getSamplesToRead() override { return 0; }
    float setGain(int) override { return 0; }
    float getGain() const override { return 0; }
    int getGainCount() override { return 0; }
    void setAgc(bool) override {}
    std::string getDescription() override { return "none"; }
};

struct Rig {
    NoController rci; NoInput in; RadioReceiver rx;
    Rig() : rx(rci, in, RadioReceiverOptions()) {}
};

} // namespace

// One receiver per process: the OFDMProcessor's constructor fills a 2 048 000-entry oscillator table.
extern "C" int ref_coarse_prs(const float* v /*2048 cf32*/, int method /*0 GetMiddle, 1 CorrelatePRS, 2 PatternOfZeros*/)
{
    static std::mutex mtx;
    static std::unique_ptr<Rig> rig;
    std::lock_guard<std::mutex> lock(mtx);
    if (!rig) rig.reset(new Rig());
    std::vector<DSPCOMPLEX> buf(2048); memcpy(buf.data(), v, 2048 * sizeof(DSPCOMPLEX));
    const FreqsyncMethod fm = method == 0 ? FreqsyncMethod::GetMiddle : method == 1 ? FreqsyncMethod::CorrelatePRS : FreqsyncMethod::PatternOfZeros;
    return rig->rx.ofdmProcessor.processPRS(buf.data(), fm);
}
