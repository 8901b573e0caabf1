// tests/native/hold_check.cpp -- self-test of the execution model's held stream (tests/hipemu: hipemu_hold_stream): toy two-stream
// programs whose result depends on a cross-stream wait.  Prints one JSON object; tests/test_emu_hold.py reads it.
#include "hip/hip_runtime.h"

__global__ void k_set(int* p, int v) { if (threadIdx.x == 0) *p = v; }
__global__ void k_copy(int* dst, const int* src) { if (threadIdx.x == 0) *dst = *src; }

// producer on stream 0, consumer on stream 1; `wait`: the consumer waits for the producer's event.  hold: -1 none, else the stream held
static int producer_consumer(bool wait, int hold)
{
    hipemu_trace_start();
    hipStream_t s[2]; hipEvent_t ev;
    hipStreamCreate(&s[0]); hipStreamCreate(&s[1]); hipEventCreate(&ev);
    int *buf, *out, host = -1;
    hipMalloc((void**)&buf, sizeof(int)); hipMalloc((void**)&out, sizeof(int));
    hipMemset(buf, 0, sizeof(int)); hipMemset(out, 0, sizeof(int));
    if (hold >= 0) hipemu_hold_stream(hold);
    hipLaunchKernelGGL(k_set, dim3(1), dim3(64), 0, s[0], buf, 7);
    hipEventRecord(ev, s[0]);
    if (wait) hipStreamWaitEvent(s[1], ev, 0);
    hipLaunchKernelGGL(k_copy, dim3(1), dim3(64), 0, s[1], out, buf);
    hipStreamSynchronize(s[1]);
    hipStreamSynchronize(s[0]);
    hipMemcpy(&host, out, sizeof(int), hipMemcpyDeviceToHost);
    hipemu_hold_none();
    hipFree(buf); hipFree(out); hipEventDestroy(ev); hipStreamDestroy(s[0]); hipStreamDestroy(s[1]);
    return host;
}

// the other covered ops on a held stream, in order: fill, host-to-device copy (source bytes taken at the call), launch, device-to-host
// copy, event record; nothing runs before the drain point, everything has run behind it.  which: 0 hipEventSynchronize, 1 hipStreamSynchronize,
// 2 hipDeviceSynchronize, 3 synchronous hipMemcpy, 4 hipFree, 5 hipStreamDestroy
static int ops_in_order(int which)
{
    hipemu_trace_start();
    hipStream_t s; hipEvent_t ev;
    hipStreamCreate(&s); hipEventCreate(&ev);
    int *buf, *out, *spare, src = 5, back = -1, dummy = 0;
    hipMalloc((void**)&buf, 2 * sizeof(int)); hipMalloc((void**)&out, sizeof(int)); hipMalloc((void**)&spare, sizeof(int));
    hipMemset(buf, 0, 2 * sizeof(int)); hipMemset(out, 0, sizeof(int));
    hipemu_hold_stream(0);
    hipMemsetAsync(buf, 0x01, sizeof(int), s);                               // buf[0] = 0x01010101
    hipMemcpyAsync(buf + 1, &src, sizeof(int), hipMemcpyHostToDevice, s);    // buf[1] = 5 ...
    src = 6;                                                                 // ... whatever the host writes there afterwards
    hipLaunchKernelGGL(k_copy, dim3(1), dim3(64), 0, s, out, buf + 1);
    hipMemcpyAsync(&back, out, sizeof(int), hipMemcpyDeviceToHost, s);
    hipEventRecord(ev, s);
    const bool nothing_yet = buf[0] == 0 && buf[1] == 0 && *out == 0 && back == -1;
    switch (which) {
        case 0: hipEventSynchronize(ev); break;
        case 1: hipStreamSynchronize(s); break;
        case 2: hipDeviceSynchronize(); break;
        case 3: hipMemcpy(&dummy, spare, sizeof(int), hipMemcpyDeviceToHost); break;
        case 4: hipFree(spare); spare = nullptr; break;
        default: break;
    }
    int r = 0;
    if (which == 5) { const int b0 = buf[0]; hipStreamDestroy(s); s = nullptr; r = nothing_yet && b0 == 0 && buf[0] == 0x01010101 && buf[1] == 5 && back == 5; }
    else r = nothing_yet && buf[0] == 0x01010101 && buf[1] == 5 && *out == 5 && back == 5;
    hipemu_hold_none();
    hipFree(buf); hipFree(out); hipFree(spare); hipEventDestroy(ev); if (s) hipStreamDestroy(s);
    return r;
}

// a wait drains only as far as the awaited record: what the held stream got behind it stays queued
static int drains_only_as_far_as_needed()
{
    hipemu_trace_start();
    hipStream_t s[2]; hipEvent_t ev;
    hipStreamCreate(&s[0]); hipStreamCreate(&s[1]); hipEventCreate(&ev);
    int* buf; hipMalloc((void**)&buf, 2 * sizeof(int)); hipMemset(buf, 0, 2 * sizeof(int));
    hipemu_hold_stream(0);
    hipLaunchKernelGGL(k_set, dim3(1), dim3(64), 0, s[0], buf, 1);
    hipEventRecord(ev, s[0]);
    hipLaunchKernelGGL(k_set, dim3(1), dim3(64), 0, s[0], buf + 1, 2);
    hipStreamWaitEvent(s[1], ev, 0);
    const bool part = buf[0] == 1 && buf[1] == 0;
    hipStreamSynchronize(s[0]);
    const bool all = buf[0] == 1 && buf[1] == 2;
    hipemu_hold_none();
    hipFree(buf); hipEventDestroy(ev); hipStreamDestroy(s[0]); hipStreamDestroy(s[1]);
    return part && all;
}

int main()
{
    printf("{\"wait_eager\": %d, \"wait_hold_producer\": %d, \"wait_hold_consumer\": %d, \"nowait_eager\": %d, \"nowait_hold_producer\": %d, \"nowait_hold_consumer\": %d",
           producer_consumer(true, -1), producer_consumer(true, 0), producer_consumer(true, 1), producer_consumer(false, -1), producer_consumer(false, 0), producer_consumer(false, 1));
    printf(", \"ops\": [%d, %d, %d, %d, %d, %d], \"partial_drain\": %d}\n", ops_in_order(0), ops_in_order(1), ops_in_order(2), ops_in_order(3), ops_in_order(4), ops_in_order(5), drains_only_as_far_as_needed());
    return 0;
}
