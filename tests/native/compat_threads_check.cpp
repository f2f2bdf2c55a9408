// compat_threads_check.cpp -- the reference-shaped entry point lanczos(stream_in, stream_out) of host/hls_compat.hpp from
// several host threads at once (its comment: "can be called repeatedly, and from several threads"; INTEGRATION.md 2: "safe under
// concurrent first calls").  Four threads are released together, so the adapter's context is created by whichever arrives first
// while the others wait for it; each then makes three calls on noise frames of its own.  Inputs and outputs go to the file named
// on the command line:
//     int32 threads, calls, in_w, in_h, out_w, out_h, channels, a;  then per (thread, call): the input bytes, the output bytes
// tests/test_concurrency_gpu.py compares every output with the CPU oracle.  Runs on the GPU; built by the test, linked against
// liblanczos_hip.so.
#define IN_WIDTH 64
#define IN_HEIGHT 48
#define OUT_WIDTH 128
#define OUT_HEIGHT 96
#define NUM_CHANNELS 3
#define LANCZOS_A 3
#include "hls_compat.hpp"

#include <condition_variable>
#include <mutex>
#include <thread>

static constexpr int kThreads = 4, kCalls = 3;
static constexpr size_t kIn = (size_t)IN_WIDTH * IN_HEIGHT * NUM_CHANNELS, kOut = (size_t)OUT_WIDTH * OUT_HEIGHT * NUM_CHANNELS;

struct Gate {   // all threads leave together
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0;
    void arrive() {
        std::unique_lock<std::mutex> l(m);
        if (++waiting == kThreads) cv.notify_all();
        else cv.wait(l, [this] { return waiting == kThreads; });
    }
};

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
        return 2;
    }
    std::vector<std::vector<uint8_t>> in(kThreads * kCalls, std::vector<uint8_t>(kIn)), out(kThreads * kCalls, std::vector<uint8_t>(kOut));
    for (int i = 0; i < kThreads * kCalls; i++) {
        uint32_t s = 12345u + 7919u * (uint32_t)i;
        for (uint8_t& b : in[i]) {
            s = s * 1664525u + 1013904223u;
            b = (uint8_t)(s >> 24);
        }
    }
    Gate gate;
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; t++)
        threads.emplace_back([&, t] {
            gate.arrive();
            for (int k = 0; k < kCalls; k++) {
                const int i = t * kCalls + k;
                hls::stream<byte_t> sin, sout;
                for (size_t p = 0; p < (size_t)IN_WIDTH * IN_HEIGHT; p++) {
                    byte_t px;
                    for (int c = 0; c < NUM_CHANNELS; c++) px.channel[c] = in[i][p * NUM_CHANNELS + c];
                    sin.write(px);
                }
                lanczos(sin, sout);
                if (!sin.empty() || sout.size() != (size_t)OUT_WIDTH * OUT_HEIGHT) {
                    std::fprintf(stderr, "thread %d call %d: %zu pixels left in, %zu out\n", t, k, sin.size(), sout.size());
                    std::exit(1);
                }
                for (size_t p = 0; p < (size_t)OUT_WIDTH * OUT_HEIGHT; p++) {
                    const byte_t px = sout.read();
                    for (int c = 0; c < NUM_CHANNELS; c++) out[i][p * NUM_CHANNELS + c] = px.channel[c];
                }
            }
        });
    for (std::thread& th : threads) th.join();
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    const int32_t head[8] = {kThreads, kCalls, IN_WIDTH, IN_HEIGHT, OUT_WIDTH, OUT_HEIGHT, NUM_CHANNELS, LANCZOS_A};
    bool ok = std::fwrite(head, sizeof(head), 1, f) == 1;
    for (int i = 0; i < kThreads * kCalls; i++)
        ok = ok && std::fwrite(in[i].data(), 1, kIn, f) == kIn && std::fwrite(out[i].data(), 1, kOut, f) == kOut;
    ok = std::fclose(f) == 0 && ok;
    std::printf("%d threads x %d calls written\n", kThreads, kCalls);
    return ok ? 0 : 2;
}
