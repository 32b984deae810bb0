// Host-side batch assembly for the training loop's input pipeline (lpi_amd/pipeline.py).  No device code.
//
// Stands in for what the reference's loop gets from torch's DataLoader: default_collate's torch.stack of the B decoded images and the pageable
// host->device copy of `images.cuda()` (methods/sprompt.py:166-167, 301).  At 11 k pairs/s a step consumes 154 MB of f32 pixels every 22 ms; one core
// moves that in 20-40 ms, so the gather into the PINNED staging buffer the DMA engine reads from is spread over a few threads.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/lpi_hip.h"

namespace {
constexpr long CHUNK = 1 << 20;      // work unit: 1 MiB of one source row (a thread takes the next unclaimed unit)
}

// dst[i * bytes_each .. ] = srcs[i][0 .. bytes_each)   for i < n, on `threads` host threads (<= 1: the calling thread alone).  Source rows may alias
// (a synthetic dataset that repeats images); dst must not overlap any source.  Returns 0, or LPI_EINVAL.
extern "C" int lpi_host_gather(void* dst, const void* const* srcs, int n, long bytes_each, int threads) {
    if (!dst || !srcs || n <= 0 || bytes_each <= 0) return LPI_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!srcs[i]) return LPI_EINVAL;
    const long per_row = (bytes_each + CHUNK - 1) / CHUNK;
    const long units = per_row * n;
    std::atomic<long> next{0};
    auto work = [&]() {
        for (;;) {
            const long u = next.fetch_add(1, std::memory_order_relaxed);
            if (u >= units) return;
            const long i = u / per_row, off = (u % per_row) * CHUNK;
            const long len = (off + CHUNK <= bytes_each) ? CHUNK : bytes_each - off;
            std::memcpy(static_cast<char*>(dst) + i * bytes_each + off, static_cast<const char*>(srcs[i]) + off, (size_t)len);
        }
    };
    int nt = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
    if ((long)nt > units) nt = (int)units;
    std::vector<std::thread> pool;
    pool.reserve(nt > 0 ? nt - 1 : 0);
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return 0;
}

// The ragged form (pixel_format='decoded': images of different sizes): dst = srcs[0][0 .. bytes[0]) ++ srcs[1][0 .. bytes[1]) ++ ..., packed without gaps,
// on `threads` host threads.  Same rules as lpi_host_gather; rows of 0 bytes are allowed.  Returns 0, or LPI_EINVAL.
extern "C" int lpi_host_gather_v(void* dst, const void* const* srcs, const long* bytes, int n, int threads) {
    if (!dst || !srcs || !bytes || n <= 0) return LPI_EINVAL;
    std::vector<long> row_off(n + 1, 0), unit_off(n + 1, 0);      // byte offset of row i in dst; first work unit of row i
    for (int i = 0; i < n; ++i) {
        if (bytes[i] < 0 || (bytes[i] > 0 && !srcs[i])) return LPI_EINVAL;
        row_off[i + 1] = row_off[i] + bytes[i];
        unit_off[i + 1] = unit_off[i] + (bytes[i] + CHUNK - 1) / CHUNK;
    }
    const long units = unit_off[n];
    std::atomic<long> next{0};
    auto work = [&]() {
        int i = 0;
        for (;;) {
            const long u = next.fetch_add(1, std::memory_order_relaxed);
            if (u >= units) return;
            while (unit_off[i + 1] <= u) ++i;           // units are claimed in increasing order: the row index only moves forward
            const long off = (u - unit_off[i]) * CHUNK;
            const long len = (off + CHUNK <= bytes[i]) ? CHUNK : bytes[i] - off;
            std::memcpy(static_cast<char*>(dst) + row_off[i] + off, static_cast<const char*>(srcs[i]) + off, (size_t)len);
        }
    };
    int nt = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
    if ((long)nt > units) nt = units > 0 ? (int)units : 1;
    std::vector<std::thread> pool;
    pool.reserve(nt - 1);
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return 0;
}
