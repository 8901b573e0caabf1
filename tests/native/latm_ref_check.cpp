// tests/native/latm_ref_check.cpp -- TEST HARNESS (tests/test_au_vs_ref.py): feeds logical frames to the reference's SuperframeFilter
// (observer, no audio decoder, no float32) with an UntouchedStreamConsumer attached, one Feed per logical frame, and prints what the
// consumer receives.
//   latm_ref_check <file of n * frame_len bytes> <frame_len>
// prints one line per forwarded LATM/LOAS frame:
//   U <feed> <duration_ms> <length> <hex bytes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dabplus_decoder.h"

namespace {
class Quiet : public SubchannelSinkObserver {};
class Consumer : public UntouchedStreamConsumer {
public:
    int feed = 0;
    void ProcessUntouchedStream(const uint8_t* data, size_t len, size_t duration_ms) override
    {
        printf("U %d %zu %zu ", feed, duration_ms, len);
        for (size_t i = 0; i < len; i++) printf("%02x", data[i]);
        printf("\n");
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
    Quiet obs;
    Consumer con;
    {
        SuperframeFilter filter(&obs, false, false);
        filter.AddUntouchedStreamConsumer(&con);
        for (size_t k = 0; (k + 1) * len <= data.size(); k++) {
            con.feed = (int)k;
            filter.Feed(data.data() + k * len, (size_t)len);
        }
        filter.RemoveUntouchedStreamConsumer(&con);
    }
    return 0;
}
