// host_copy.h -- a list of byte ranges copied by several threads (plain C++17, no HIP).  The host-buffer terrain path moves the
// caller's rows into pinned staging and the planes back with it: caller's memory is pageable, fresh output pages fault on first
// touch -- both want many threads.
#pragma once
#include <stddef.h>
#include <string.h>

#include <thread>
#include <vector>

struct XdSpan { char* dst; const char* src; size_t bytes; };

constexpr size_t XD_COPY_THREADED_FROM = (size_t)4 << 20;   // below this total one thread copies: starting threads costs more

// The spans laid end to end are cut into `nthreads` equal byte shares, one per thread, whatever the span borders.
inline void xd_parallel_copy(const std::vector<XdSpan>& spans, int nthreads) {
    size_t total = 0;
    for (const XdSpan& sp : spans) total += sp.bytes;
    if (total < XD_COPY_THREADED_FROM || nthreads <= 1) {
        for (const XdSpan& sp : spans) memcpy(sp.dst, sp.src, sp.bytes);
        return;
    }
    std::vector<std::thread> workers;
    const size_t per = (total + (size_t)nthreads - 1) / (size_t)nthreads;
    for (int t = 0; t < nthreads; ++t)
        workers.emplace_back([&, t]() {
            size_t lo = per * (size_t)t, hi = lo + per < total ? lo + per : total, pos = 0;
            for (const XdSpan& sp : spans) {
                const size_t a = pos > lo ? pos : lo, b = pos + sp.bytes < hi ? pos + sp.bytes : hi;
                if (b > a) memcpy(sp.dst + (a - pos), sp.src + (a - pos), b - a);
                pos += sp.bytes;
                if (pos >= hi) break;
            }
        });
    for (auto& w : workers) w.join();
}
