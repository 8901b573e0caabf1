// oracle/sort_order.cpp -- TEST INFRASTRUCTURE.  EarliestPeakWithBinning sorts its 102 bin peaks with std::sort (phasereference.cpp:172-175)
// and keeps the first four that lie within 500 samples of the first one: among bit-identical peaks -- equal echoes of a single-frequency
// network give them -- the bins it keeps are the ones the C++ library's sort happens to leave in front.  That order belongs to the
// library the reference is built with, so the restatement asks the same std::sort, with the reference's element type and comparison,
// instead of imitating it (oracle/tii_order.cpp does the same for the TII decoder's unordered_map).
#include <algorithm>
#include <utility>
#include <vector>

extern "C" void orc_std_sort_desc(const float* value, const int* index, int n, int* order /* [n]: bin numbers, highest peak first */)
{
    struct peak_t { int index = -1; float value = 0; int bin = 0; };
    std::vector<peak_t> bins;
    for (int k = 0; k < n; k++) { peak_t p; p.index = index[k]; p.value = value[k]; p.bin = k; bins.push_back(std::move(p)); }
    std::sort(bins.begin(), bins.end(), [&](const peak_t& lhs, const peak_t& rhs) { return lhs.value > rhs.value; });
    for (int k = 0; k < n; k++) order[k] = bins[k].bin;
}
