// Kernel microbenchmarks (scripts/bench_gemv.py, bench_gemm.py, bench_attn.py): each cycles
// `copies` operand sets through a graph of `iters` launches so the 256 MB Infinity Cache cannot
// serve them, and returns microseconds per launch.
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "engine.h"
#include "host_harness.h"
#include "kernels.h"

namespace dl {

double benchGemvQ40(int rows, int n, int pro, int epi, int B, int lanes, int passes, int copies, int iters,
                    std::vector<unsigned long long> *trace) {
    Scratch sc;
    hipStream_t s = sc.s;
    // (allocRaw: the weight copies and the outputs are written whole, a memset would only slow set-up)
    const int L = lanes > 0 ? lanes : hipk::gemvLanesPerRow(n, rows, B, true);
    const hipk::Q40Tiling t = hipk::q40Tiling(rows, n, L);
    std::vector<uint8_t *> qs(copies);
    std::vector<uint16_t *> d(copies);
    for (int c = 0; c < copies; c++) {
        qs[c] = sc.allocRaw<uint8_t>(t.qsBytes);
        d[c] = sc.allocRaw<uint16_t>(t.dBytes / 2);
        hipk::launchFillQ40(qs[c], d[c], t.qsBytes / 16, 0.01f, 77 + c, s);
    }
    float *x = sc.allocRaw<float>((size_t)B * n), *y = sc.allocRaw<float>((size_t)B * n);
    float *xn = sc.allocRaw<float>((size_t)B * n), *w = sc.allocRaw<float>(n);
    hipk::launchFillF32Uniform(x, (size_t)B * n, 1.f, 1, s);
    hipk::launchFillF32Uniform(y, (size_t)B * n, 1.f, 2, s);
    hipk::launchFillF32Const(w, n, 1.f, s);
    int8_t *aq = sc.allocRaw<int8_t>((size_t)B * n);
    float2 *as = sc.alloc<float2>((size_t)B * n / 32);
    DL_HIP(hipMemsetAsync(aq, 1, (size_t)B * n, s));
    const int outRows = epi == hipk::EPI_ACT_Q80 ? rows / 2 : rows;
    float *out = sc.allocRaw<float>((size_t)B * rows);
    int8_t *oq = sc.allocRaw<int8_t>((size_t)B * outRows);
    float2 *os = sc.allocRaw<float2>((size_t)B * outRows / 32);
    hipk::GemvArgs a;
    a.rows = rows;
    a.n = n;
    a.lanes = L;
    a.passes = passes > 0 ? passes : hipk::gemvDefaultPasses(n, rows, B, true, epi);
    if (passes <= 0 && lanes > 0) {  // forced lane count: same residency rule with its rows/pass
        const int rp = 256 / lanes * 2, grid0 = (rows + rp - 1) / rp;
        a.passes = (grid0 + 511) / 512;
        if (epi == hipk::EPI_ACT_Q80)
            while ((rp * a.passes) % 64) a.passes++;
    }
    a.in = x;
    a.ldIn = n;
    a.addIn = y;
    a.xNext = xn;
    a.normW = w;
    a.aq = aq;
    a.as = as;
    a.out = out;
    a.ldOut = outRows;
    a.oq = oq;
    a.os = os;
    if (epi == hipk::EPI_QKV) {  // Llama-like split: q = 2/3 of the rows, k = v = 1/6, one position
        a.hs = 128;
        a.kv0 = rows / 6;
        a.q0 = rows - 2 * a.kv0;
        a.seqLen = 1;
        a.kvBf16 = 1;
        const int *zeros = sc.alloc<int>(64);
        a.rope = sc.alloc<float2>(64);
        a.pos = zeros;
        a.slot = zeros;
        a.kcache = sc.allocRaw<uint16_t>(a.kv0);
        a.vcache = sc.allocRaw<uint16_t>(a.kv0);
    }
    if (epi == hipk::EPI_STORE_TP) {  // the TP tail in loopback (ComputeOnlyComm's exchange):
        // DL_BENCH_TP_WORLD ranks (default 8), DL_BENCH_TP_Q80=0 for the f32 wire format
        const char *w = std::getenv("DL_BENCH_TP_WORLD"), *q = std::getenv("DL_BENCH_TP_Q80");
        a.tp.world = w ? std::atoi(w) : 8;
        a.tp.q80 = q && *q == '0' ? 0 : 1;
        a.tp.loopback = 1;
        a.tp.stride = (long long)B * rows * 9;
        a.tp.epochs = sc.alloc<unsigned>((size_t)a.tp.stride);
        a.tp.error = sc.alloc<int>(1);
        if (a.tp.q80 && passes <= 0)  // whole Q80 blocks of 32 rows per workgroup (engine tpPasses)
            while ((256 / L * 2 * a.passes) % 32) a.passes++;
    }
    const int grid = (rows + (256 / L) * 2 * a.passes - 1) / ((256 / L) * 2 * a.passes);
    unsigned long long *tbuf = trace ? sc.allocRaw<unsigned long long>((size_t)iters * grid * 8) : nullptr;
    const double us = timeGraphUs(s, iters, [&](int c) {
        a.qs = qs[c % copies];
        a.wd = d[c % copies];
        a.trace = tbuf ? tbuf + (size_t)c * grid * 8 : nullptr;
        hipk::launchGemv(a, B, pro, epi, true, s);
    });
    if (trace) *trace = sc.download(tbuf, (size_t)iters * grid * 8);
    return us;
}

double benchGemmQ40(int rows, int n, int M, int epi, int copies, int iters, std::vector<unsigned long long> *trace) {
    DL_CHECK(M >= 1 && M <= hipk::kGemmMaxTokens && hipk::gemmSupported(n) && rows % 64 == 0, "bad gemm bench shape");
    Scratch sc;
    hipStream_t s = sc.s;
    const int L = hipk::gemvLanesPerRow(n, rows, 1, true);
    const hipk::Q40Tiling t = hipk::q40Tiling(rows, n, L);
    std::vector<uint8_t *> qs(copies);
    std::vector<uint16_t *> d(copies);
    for (int c = 0; c < copies; c++) {
        qs[c] = sc.alloc<uint8_t>(t.qsBytes);
        d[c] = sc.alloc<uint16_t>(t.dBytes / 2);
        hipk::launchFillQ40(qs[c], d[c], t.qsBytes / 16, 0.01f, 77 + c, s);
    }
    // the operand rows a launch reads: the narrow kernel's 16/32/64/128-row pad, the wide kernel's
    // whole 128-token tiles
    const int MP = hipk::gemmUsesWide(M) ? (M + 127) / 128 * 128 : hipk::gemmTokenPad(M);
    _Float16 *x = sc.alloc<_Float16>((size_t)MP * n);
    hipk::launchFillF32Uniform((float *)x, (size_t)MP * n / 2, 1e-3f, 3, s);  // small finite f16 pairs
    const size_t part = hipk::gemmPartFloats(rows, n, M);
    hipk::GemmArgs g;
    g.e.rows = rows;
    g.e.n = n;
    g.e.lanes = L;
    g.e.out = sc.alloc<float>((size_t)M * rows);
    g.e.ldOut = epi == hipk::EPI_STORE ? rows : rows / 2;
    g.outH = sc.alloc<_Float16>((size_t)M * rows);
    g.x = x;
    g.M = M;
    g.splits = hipk::gemmSplits(rows, n, M, L);
    g.part = part ? sc.alloc<float>(part) : nullptr;
    g.counters = sc.alloc<int>((size_t)std::max(rows / 64 + 1, hipk::gemmCounterInts(rows, M)));
    auto launch = [&](int c) {
        g.e.qs = qs[c % copies];
        g.e.wd = d[c % copies];
        hipk::launchGemmQ40(g, epi, s);
    };
    const double us = timeGraphUs(s, iters, launch);
    if (trace) {  // one more (eager) launch with per-workgroup stamps
        const size_t words = 8 * (size_t)((rows + 63) / 64) * g.splits;
        g.e.trace = sc.alloc<unsigned long long>(words);
        launch(1);
        *trace = sc.download(g.e.trace, words);
    }
    return us;
}

double benchAttention(int nHeads0, int kvMul, int hs, int seqLen, int pos, int B, int copies, int iters,
                      std::vector<unsigned long long> *trace, bool kvBf16) {
    DL_CHECK(kvMul >= 1 && nHeads0 % kvMul == 0 && pos >= 0 && pos < seqLen && B >= 1, "bad attention bench shape");
    Scratch sc;
    hipStream_t s = sc.s;
    const int kv0 = nHeads0 / kvMul * hs, q0 = nHeads0 * hs;
    const size_t kvElems = (size_t)B * seqLen * kv0;  // one slot per row
    std::vector<float *> kc(copies), vc(copies);
    const size_t kvWords = kvBf16 ? kvElems / 2 : kvElems;  // bf16 pairs of small values, or f32
    for (int c = 0; c < copies; c++) {
        kc[c] = sc.alloc<float>(kvWords);
        vc[c] = sc.alloc<float>(kvWords);
        hipk::launchFillF32Uniform(kc[c], kvWords, 1.f, 5 + c, s);
        hipk::launchFillF32Uniform(vc[c], kvWords, 1.f, 9 + c, s);
    }
    float *q = sc.alloc<float>((size_t)B * q0);
    hipk::launchFillF32Uniform(q, (size_t)B * q0, 1.f, 3, s);
    std::vector<int> hp(B), hsl(B);
    for (int b = 0; b < B; b++) hp[b] = pos, hsl[b] = b;
    hipk::AttnArgs a;
    a.q = q;
    a.ldq = q0;
    a.pos = sc.upload(hp);
    a.slot = sc.upload(hsl);
    a.nHeads0 = nHeads0;
    a.kvMul = kvMul;
    a.hs = hs;
    a.kv0 = kv0;
    a.seqLen = seqLen;
    a.splitGrid = hipk::attnSplitGrid(seqLen);
    a.chunkMax = hipk::attnChunkMax(seqLen, a.splitGrid);
    a.chunkMin = hipk::attnChunkMin();
    a.partO = sc.alloc<float>((size_t)B * nHeads0 * a.splitGrid * hs);
    a.partML = sc.alloc<float>((size_t)B * nHeads0 * a.splitGrid * 2);
    a.outQ = sc.alloc<int8_t>((size_t)B * q0);
    a.outS = sc.alloc<float2>((size_t)B * q0 / 32);
    a.ldOut = q0;
    a.kvBf16 = kvBf16 ? 1 : 0;
    a.counters = sc.alloc<int>((size_t)B * nHeads0);
    DL_HIP(hipStreamSynchronize(s));
    auto launch = [&](int c) {
        a.kcache = kc[c % copies];
        a.vcache = vc[c % copies];
        hipk::launchAttention(a, B, s);
    };
    const double us = timeGraphUs(s, iters, launch);
    if (trace) {  // one more (eager) launch with per-workgroup stamps (MFMA decode kernel)
        const size_t words = 8 * (size_t)(nHeads0 / kvMul) * a.splitGrid * B;
        a.trace = sc.alloc<unsigned long long>(words);
        launch(iters);
        *trace = sc.download(a.trace, words);
    }
    return us;
}

}  // namespace dl

namespace dl {

// The separate-collective schedule of a tensor-parallel forward (engine_forward.cpp: per layer two
// Q80-rounded all-reduces of [rows][dim] partial sums, then the logits slices gathered to the root
// and the argmax winner pairs all-gathered), on `comm`, run eagerly or captured once into a hipGraph
// and replayed. Rank r contributes c * k(r, i) with integer k and c = 2^-4 (every Q80 block holds a
// 127 * c element, so the Q80 round trip and the sums are exact); returns the largest |got - want|
// over every output of every run (0 when the transport is right), checked on the host.
double commScheduleCheck(DeviceComm &comm, int layers, int rows, int dim, int vocab0, int runs, bool graph) {
    DL_CHECK(layers >= 1 && rows >= 1 && dim % 32 == 0 && vocab0 >= 1 && runs >= 1, "bad schedule shape");
    const int W = comm.size(), me = comm.rank();
    const float c = 1.0f / 16.0f;
    auto k = [](int r, size_t i) { return (i % 32) == 0 ? 127.f : (float)((int)((i * 37 + (size_t)r * 11) % 255) - 127); };
    const size_t ny = (size_t)rows * dim, nl = (size_t)rows * vocab0, np = 2 * (size_t)rows;
    std::vector<float> hy(ny), hl(nl), hp(np);
    for (size_t i = 0; i < ny; i++) hy[i] = c * k(me, i);
    for (size_t i = 0; i < nl; i++) hl[i] = (float)(me * 1000 + (int)(i % 997));
    for (size_t i = 0; i < np; i++) hp[i] = (float)(me * 7 + (int)i);
    Scratch sc;
    hipStream_t s = sc.s;
    float *ySrc = sc.upload(hy), *y = sc.alloc<float>(ny), *outs = sc.alloc<float>(ny * layers);
    float *lg = sc.upload(hl), *lgAll = sc.alloc<float>(nl * W), *pr = sc.upload(hp), *prAll = sc.alloc<float>(np * W);
    auto schedule = [&]() {
        for (int l = 0; l < layers; l++) {
            DL_HIP(hipMemcpyAsync(y, ySrc, ny * 4, hipMemcpyDeviceToDevice, s));
            hipk::launchQ80Roundtrip(y, ny, s);
            comm.allReduceSum(y, ny, s);
            DL_HIP(hipMemcpyAsync(outs + (size_t)l * ny, y, ny * 4, hipMemcpyDeviceToDevice, s));
        }
        comm.gatherToRoot(lg, lgAll, nl, s);
        comm.allGather(pr, prAll, np, s);
    };
    CapturedGraph captured;
    if (graph) captured.capture(s, schedule);
    double err = 0;
    std::vector<float> got;
    for (int run = 0; run < runs; run++) {
        DL_HIP(hipMemsetAsync(outs, 0, ny * layers * 4, s));
        DL_HIP(hipMemsetAsync(lgAll, 0, nl * W * 4, s));
        DL_HIP(hipMemsetAsync(prAll, 0, np * W * 4, s));
        if (graph)
            captured.launch(s);
        else
            schedule();
        got = sc.download(outs, ny * layers);
        for (int l = 0; l < layers; l++)
            for (size_t i = 0; i < ny; i++) {
                float want = 0;
                for (int r = 0; r < W; r++) want += c * k(r, i);
                err = std::max(err, (double)std::fabs(got[(size_t)l * ny + i] - want));
            }
        if (me == 0) {
            got = sc.download(lgAll, nl * W);
            for (int r = 0; r < W; r++)
                for (size_t i = 0; i < nl; i++)
                    err = std::max(err, (double)std::fabs(got[r * nl + i] - (float)(r * 1000 + (int)(i % 997))));
        }
        got = sc.download(prAll, np * W);
        for (int r = 0; r < W; r++)
            for (size_t i = 0; i < np; i++) err = std::max(err, (double)std::fabs(got[r * np + i] - (float)(r * 7 + (int)i)));
    }
    return err;
}

// Yardstick of the prefix copy (scripts/bench_prefix.py): `iters` device-to-device hipMemcpyAsync
// copies of `bytes` between two buffers on one stream, timed by events after two warm-up copies.
double benchMemcpyD2D(size_t bytes, int iters) {
    Scratch sc;
    uint8_t *a = sc.allocRaw<uint8_t>(bytes), *b = sc.allocRaw<uint8_t>(bytes);
    DL_HIP(hipMemsetAsync(a, 1, bytes, sc.s));
    return timeEagerUs(sc.s, iters, 2, [&] { DL_HIP(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, sc.s)); });
}

}  // namespace dl
