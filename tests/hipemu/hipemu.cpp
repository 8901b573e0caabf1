// tests/hipemu/hipemu.cpp -- TEST INFRASTRUCTURE: fiber scheduler behind tests/hipemu/hip/hip_runtime.h.
#include "hip/hip_runtime.h"
#include <stdexcept>
#include <mutex>
#include <set>
#include <algorithm>
#include <string>
#include <utility>
#include <deque>

hipemu_idx threadIdx, blockIdx, blockDim, gridDim;

namespace {
constexpr size_t STACK = 512 * 1024;
// minimal x86-64 System V context switch (callee-saved registers + stack pointer); ucontext's swapcontext makes two
// sigprocmask system calls per switch, which dominated the run time of barrier-heavy kernels
struct Fiber { void* sp = nullptr; char* stack = nullptr; bool done = true; hipemu_idx tid; };
extern "C" void hipemu_switch(void** save_sp, void* load_sp);
asm(R"(
.text
.globl hipemu_switch
.type hipemu_switch,@function
hipemu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
.size hipemu_switch,.-hipemu_switch
)");
struct Block {
    std::vector<Fiber> f; int cur = -1; int nlive = 0;
    int arrived = 0; unsigned gen = 0;
    // wave state
    int w_arrived[16]; unsigned w_gen[16]; unsigned w_val[2][16][64]; unsigned w_tog[16][64]; bool w_pred[16][64]; int w_live[16];
};
Block B;
void* sched_sp = nullptr;
const std::function<void()>* g_body = nullptr;

void fiber_main() {
    (*g_body)();
    Fiber& me = B.f[B.cur];
    me.done = true; B.nlive--; B.w_live[B.cur / 64]--;
    hipemu_switch(&me.sp, sched_sp);
    __builtin_unreachable();
}
void yield_() { Fiber& me = B.f[B.cur]; hipemu_switch(&me.sp, sched_sp); }
}

void hipemu_syncthreads() {
    unsigned gen = B.gen;
    if (++B.arrived >= B.nlive) { B.arrived = 0; B.gen++; }
    else while (B.gen == gen) yield_();
}

static void wave_barrier(int w) {
    unsigned gen = B.w_gen[w];
    if (++B.w_arrived[w] >= B.w_live[w]) { B.w_arrived[w] = 0; B.w_gen[w]++; }
    else while (B.w_gen[w] == gen) yield_();
}

unsigned hipemu_wave_exchange_impl(unsigned v, int src_lane, bool) {
    // double-buffered: a lane can only reach its second-next exchange after every lane has left this one
    int t = B.cur, w = t / 64, l = t & 63;
    const unsigned tog = (B.w_tog[w][l]++) & 1;
    B.w_val[tog][w][l] = v;
    wave_barrier(w);
    return B.w_val[tog][w][src_lane & 63];
}

unsigned long long hipemu_ballot_impl(bool p) {
    int t = B.cur, w = t / 64, l = t & 63;
    B.w_pred[w][l] = p;
    wave_barrier(w);
    unsigned long long m = 0;
    int n = (int)B.f.size() - w * 64; if (n > 64) n = 64;
    for (int i = 0; i < n; i++) if (B.w_pred[w][i] && !B.f[w * 64 + i].done) m |= 1ull << i;
    wave_barrier(w);
    return m;
}

// One kernel at a time: the model keeps its block state (and the statics that stand in for LDS) in globals.  Host code with several
// threads (welle.io_amd/host/gpu_node_receiver.cpp: one per shard) then simply takes turns, kernel by kernel.
static std::mutex g_launch_mutex;
void hipemu_launch(dim3 grid, dim3 block, const std::function<void()>& body) {
    std::lock_guard<std::mutex> one_at_a_time(g_launch_mutex);
    const int nt = (int)(block.x * block.y * block.z);
    if (nt > 1024) throw std::runtime_error("hipemu: block too large");
    if ((int)B.f.size() < nt) {
        size_t old = B.f.size(); B.f.resize(nt);
        for (size_t i = old; i < B.f.size(); i++) B.f[i].stack = (char*)malloc(STACK);
    }
    g_body = &body;
    gridDim = {grid.x, grid.y, grid.z}; blockDim = {block.x, block.y, block.z};
    for (unsigned bz = 0; bz < grid.z; bz++) for (unsigned by = 0; by < grid.y; by++) for (unsigned bx = 0; bx < grid.x; bx++) {
        B.nlive = nt; B.arrived = 0; B.gen = 0;
        memset(B.w_tog, 0, sizeof B.w_tog);
        for (int w = 0; w < 16; w++) { B.w_arrived[w] = 0; B.w_gen[w] = 0; int n = nt - 64 * w; B.w_live[w] = n < 0 ? 0 : (n > 64 ? 64 : n); }
        for (int t = 0; t < nt; t++) {
            Fiber& f = B.f[t];
            // initial frame: six zeroed callee-saved registers, then the entry address; rsp after the `ret` into
            // fiber_main must be 8 mod 16 as after a call
            uintptr_t top = ((uintptr_t)f.stack + STACK) & ~(uintptr_t)15;
            void** sp = (void**)(top - 8);
            *--sp = (void*)fiber_main;
            for (int k = 0; k < 6; k++) *--sp = nullptr;
            f.sp = sp;
            f.done = false;
            f.tid = {t % block.x, (t / block.x) % block.y, t / (block.x * block.y)};
        }
        while (B.nlive > 0) {
            for (int t = 0; t < nt; t++) {
                if (B.f[t].done) continue;
                B.cur = t; threadIdx = B.f[t].tid; blockIdx = {bx, by, bz};
                hipemu_switch(&sched_sp, B.f[t].sp);
            }
        }
    }
    g_body = nullptr;
}

// ---- what is alive: device blocks, page-locked blocks, streams, events.  A stream is a distinct non-null object (two fields of a handle
// that name the same stream compare equal, two streams never do); releasing what is not alive -- a second time, or something never
// created -- aborts with a message.
namespace {
enum { LIVE_DEV = 0, LIVE_HOST, LIVE_STREAM, LIVE_EVENT, LIVE_KINDS };
const char* const live_name[LIVE_KINDS] = {"hipFree", "hipHostFree", "hipStreamDestroy", "hipEventDestroy"};
std::mutex g_live_mutex;
std::set<const void*> g_live[LIVE_KINDS];
std::vector<std::pair<int64_t, int64_t>> g_stream_log;
struct StreamObj { unsigned flags; int priority; int64_t id; };
int64_t g_events_created = 0;
// queue-order trace (hip_runtime.h): the text so far, and the creation counts at hipemu_trace_start that stream / event names count from
bool g_trace_on = false; std::string g_trace; int64_t g_trace_stream0 = 0, g_trace_event0 = 0;

void born(int kind, const void* p) { std::lock_guard<std::mutex> l(g_live_mutex); g_live[kind].insert(p); }
void gone(int kind, const void* p)
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    if (g_live[kind].erase(p) == 1) return;
    fprintf(stderr, "hipemu: %s(%p): not alive (released twice, or never created)\n", live_name[kind], p);
    abort();
}
hipError_t new_block(int kind, void** p, size_t n)
{
    *p = aligned_alloc(256, (n + 255) / 256 * 256 + 256);
    if (!*p) return 2;
    born(kind, *p);
    return hipSuccess;
}
hipError_t new_stream(hipStream_t* s, unsigned flags, int priority)
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    *s = new StreamObj{flags, priority, (int64_t)g_stream_log.size()};
    g_live[LIVE_STREAM].insert(*s);
    g_stream_log.emplace_back((int64_t)flags, (int64_t)priority);
    return hipSuccess;
}
}

hipError_t hipMalloc(void** p, size_t n) { return new_block(LIVE_DEV, p, n); }
hipError_t hipFree(void* p) { hipemu_drain(); if (p) { gone(LIVE_DEV, p); free(p); } return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return new_block(LIVE_HOST, p, n); }
hipError_t hipHostFree(void* p) { hipemu_drain(); if (p) { gone(LIVE_HOST, p); free(p); } return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s) { return new_stream(s, 0, 0); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return new_stream(s, flags, 0); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) { return new_stream(s, flags, priority); }
hipError_t hipStreamDestroy(hipStream_t s) { if (hipemu_held(s)) hipemu_hold_none(); gone(LIVE_STREAM, s); delete static_cast<StreamObj*>(s); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e)
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    *e = new hipemu_event{{}, g_events_created++, 0};
    g_live[LIVE_EVENT].insert(*e);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { hipemu_drain_event(e); gone(LIVE_EVENT, e); delete e; return hipSuccess; }

extern "C" void hipemu_live_counts(int64_t out[4])
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    for (int k = 0; k < LIVE_KINDS; k++) out[k] = (int64_t)g_live[k].size();
}
extern "C" int64_t hipemu_stream_creations(int64_t* flags_priority, int64_t cap)
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    for (int64_t i = 0; i < cap && i < (int64_t)g_stream_log.size(); i++) { flags_priority[2 * i] = g_stream_log[i].first; flags_priority[2 * i + 1] = g_stream_log[i].second; }
    return (int64_t)g_stream_log.size();
}

extern "C" void hipemu_trace_start()
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    g_trace_on = true; g_trace.clear(); g_trace_stream0 = (int64_t)g_stream_log.size(); g_trace_event0 = g_events_created;
}
extern "C" int64_t hipemu_trace_read(char* text, int64_t cap)
{
    std::lock_guard<std::mutex> l(g_live_mutex);
    if (text && cap > 0) memcpy(text, g_trace.data(), std::min<size_t>((size_t)cap, g_trace.size()));
    return (int64_t)g_trace.size();
}
void hipemu_trace_op(const char* op, hipStream_t s, hipEvent_t e, const char* kernel, dim3 grid, dim3 block, size_t bytes)
{
    if (!g_trace_on) return;
    std::lock_guard<std::mutex> l(g_live_mutex);
    auto name = [](char c, bool null, int64_t id) { return null ? std::string("-") : id < 0 ? std::string(1, c) + "?" : c + std::to_string(id); };
    char dims[96] = "- -";
    if (kernel) snprintf(dims, sizeof dims, "%ux%ux%u %ux%ux%u", grid.x, grid.y, grid.z, block.x, block.y, block.z);
    g_trace += std::string(op) + " " + name('s', !s, s ? static_cast<StreamObj*>(s)->id - g_trace_stream0 : 0) + " " + name('e', !e, e ? e->id - g_trace_event0 : 0) + " "
             + (kernel ? kernel : "-") + " " + dims + " " + (bytes ? std::to_string(bytes) : std::string("-")) + "\n";
}

// ---- one held stream (hip_runtime.h): its ops wait here, in order, until something the runtime orders behind them is met
namespace {
struct HeldOp { std::function<void()> run; hipEvent_t recorded; };
std::deque<HeldOp> g_held;
int64_t g_hold_index = -1;
void run_front()
{
    HeldOp op = std::move(g_held.front());
    g_held.pop_front();
    op.run();
    if (op.recorded) op.recorded->queued--;
}
}
bool hipemu_held(hipStream_t st) { return st && g_hold_index >= 0 && static_cast<StreamObj*>(st)->id - g_trace_stream0 == g_hold_index; }
void hipemu_defer(std::function<void()> op, hipEvent_t recorded)
{
    if (recorded) recorded->queued++;
    g_held.push_back(HeldOp{std::move(op), recorded});
}
void hipemu_drain() { while (!g_held.empty()) run_front(); }
void hipemu_drain_event(hipEvent_t e) { while (e && e->queued > 0) run_front(); }
void hipemu_launch_on(hipStream_t st, dim3 grid, dim3 block, std::function<void()> body)
{
    if (hipemu_held(st)) hipemu_defer([grid, block, body = std::move(body)]() { hipemu_launch(grid, block, body); });
    else hipemu_launch(grid, block, body);
}
extern "C" void hipemu_hold_stream(int64_t index) { hipemu_drain(); g_hold_index = index; }
extern "C" void hipemu_hold_none() { hipemu_drain(); g_hold_index = -1; }
