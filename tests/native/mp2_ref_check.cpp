// tests/native/mp2_ref_check.cpp -- TEST HARNESS (tests/test_mp2_vs_ref.py): feeds logical frames to the reference's MP2Decoder, one Feed
// per logical frame as DecoderAdapter::addtoFrame does, and records what its SubchannelSinkObserver sees.
//   mp2_ref_check <file of n * frame_len bytes> <frame_len>
// prints one line per frame the decoder returned and one per Feed:
//   E <feed> <new_format> <crc_ok> <fpad0> <fpad1> <xpad_len> <body0> <body1> <body2> <body3>
//   F <feed> <audio errors of that Feed>             (the value onFrameErrors reports after that logical frame)
//   T <feed>                                          (the Feed threw; nothing after it is recorded)
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>
#include "dab_decoder.h"

namespace {
struct Rec {
    int feed, new_format, crc_ok, fpad0, fpad1, xpad_len, b[4];
};

class Recorder : public SubchannelSinkObserver {
public:
    std::vector<Rec> ev;
    int feed = 0, errors = 0;
    bool pending_format = false;
    void FormatChange(const AUDIO_SERVICE_FORMAT&) override { pending_format = true; }
    void ProcessPAD(const uint8_t* xpad, size_t xpad_len, bool, const uint8_t* fpad) override
    {
        Rec r{feed, pending_format ? 1 : 0, 1, fpad[0], fpad[1], (int)xpad_len, {xpad[0], xpad[1], xpad[2], xpad[3]}};
        pending_format = false;
        ev.push_back(r);
    }
    void AudioError(const std::string&) override
    {
        errors++;
        if (!ev.empty()) ev.back().crc_ok = 0;
    }
};
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s frames.bin frame_len\n", argv[0]); return 2; }
    const long len = atol(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    if (!f || len <= 0) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    Recorder rec;
    {
        MP2Decoder dec(&rec, false);
        for (size_t k = 0; (k + 1) * len <= data.size(); k++) {
            rec.feed = (int)k;
            rec.errors = 0;
            size_t before = rec.ev.size();
            bool threw = false;
            try { dec.Feed(data.data() + k * len, (size_t)len); } catch (const std::exception&) { threw = true; }
            for (size_t i = before; i < rec.ev.size(); i++) {
                const Rec& r = rec.ev[i];
                printf("E %d %d %d %d %d %d %d %d %d %d\n", r.feed, r.new_format, r.crc_ok, r.fpad0, r.fpad1, r.xpad_len, r.b[0], r.b[1], r.b[2], r.b[3]);
            }
            if (threw) { printf("T %d\n", (int)k); break; }
            printf("F %d %d\n", (int)k, rec.errors);
        }
    }
    return 0;
}
