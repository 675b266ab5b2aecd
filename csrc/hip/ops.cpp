// Single-kernel entry points (see ops.h). Host staging is deliberately simple: synchronous copies,
// one allocation per operand, freed on return.
#include "ops.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <tuple>

#include "../core/quant.h"
#include "device_comm.h"
#include "host_harness.h"
#include "kernels.h"

namespace dl {
namespace ops {

namespace {

// File-layout Q40 blocks -> the engine's tiled device layout (csrc/hip/kernels.h Q40Tiling).
struct DevQ40 {
    uint8_t *qs = nullptr;
    uint16_t *d = nullptr;
    int lanes = 0;
};

constexpr size_t kLdsLimit = 160 * 1024;  // LDS of a gfx950 CU

void checkLanes(int lanes) {
    DL_CHECK(lanes == 0 || lanes == 16 || lanes == 32 || lanes == 64, "gemv lanes must be 0 (auto), 16, 32 or 64");
}

// Launch geometry of a Q40 ring GEMV op: the forced (or default) lanes per row and passes, the
// rows one workgroup covers, and the refusal of a launch the kernel cannot run.
struct Q40Geom {
    int lanes = 0, passes = 0, wgRows = 0;
};
Q40Geom q40Geom(int rows, int n, int B, int epi, int lanes, int passes) {
    checkLanes(lanes);
    DL_CHECK(rows > 0 && n > 0 && n % 32 == 0, "Q40 shape");
    DL_CHECK(passes >= 0, "gemv passes must be 0 (default) or >= 1");
    Q40Geom g;
    g.lanes = lanes > 0 ? lanes : hipk::gemvLanesPerRow(n, rows, 1, true);
    g.passes = passes > 0 ? passes : hipk::gemvDefaultPasses(n, rows, B, true, epi, g.lanes);
    g.wgRows = 256 / g.lanes * hipk::gemvRowGroup(B, true) * g.passes;
    DL_CHECK(hipk::gemvLdsBytes(n, B, true, g.wgRows, hipk::PRO_RESNORM) <= kLdsLimit,
             "gemv LDS footprint beyond the device limit");
    DL_CHECK(epi != hipk::EPI_ACT_Q80 || g.wgRows % 64 == 0,
             "gemv SwiGLU -> Q80: rows per workgroup must be a multiple of 64 (whole Q80 blocks)");
    return g;
}

DevQ40 uploadQ40(Scratch &sc, const std::vector<uint8_t> &blocks, int rows, int n, int lanes = 0) {
    DL_CHECK(n % 32 == 0 && rows > 0, "Q40 shape");
    checkLanes(lanes);
    const size_t nb = (size_t)rows * (n / 32);
    DL_CHECK(blocks.size() == nb * sizeof(BlockQ40), "Q40 blocks size");
    std::vector<uint8_t> qs(nb * 16);
    std::vector<uint16_t> d(nb);
    const BlockQ40 *b = reinterpret_cast<const BlockQ40 *>(blocks.data());
    for (size_t i = 0; i < nb; i++) {
        std::memcpy(&qs[i * 16], b[i].qs, 16);
        d[i] = b[i].d;
    }
    DevQ40 m;
    m.lanes = lanes > 0 ? lanes : hipk::gemvLanesPerRow(n, rows, 1, true);
    const hipk::Q40Tiling t = hipk::q40Tiling(rows, n, m.lanes);
    std::vector<uint8_t> qt(t.qsBytes);
    std::vector<uint32_t> dt(t.dBytes / 4);
    hipk::tileQ40(qs.data(), d.data(), rows, n, m.lanes, qt.data(), dt.data());
    m.qs = sc.upload(qt);
    m.d = reinterpret_cast<uint16_t *>(sc.upload(dt));
    return m;
}

// The [kv0] cache row of (slot[b], pos[b]) for every b from a head-major cache preset to the guard
// pattern as a whole (f32 view of the bf16 or f32 elements); throws when any other element changed.
void appendedRows(Scratch &sc, const uint8_t *cache, size_t cacheElems, int seqLen, int kv0, int hs,
                  const std::vector<int> &pos, const std::vector<int> &slot, bool kvBf16, const char *what,
                  std::vector<float> *out) {
    const size_t eb = kvBf16 ? 2 : 4;
    const int B = (int)pos.size();
    std::vector<uint8_t> all = sc.download(cache, cacheElems * eb);
    out->assign((size_t)B * kv0, 0.f);
    for (int b = 0; b < B; b++)
        for (int kh = 0; kh < kv0 / hs; kh++) {
            const size_t off = hipk::kvOff(hipk::KvMap{}, seqLen, kv0 / hs, hs, slot[b], pos[b], kh);
            for (int i = 0; i < hs; i++) {
                uint32_t u = 0;
                if (kvBf16) {
                    uint16_t h;
                    std::memcpy(&h, &all[(off + i) * 2], 2);
                    u = (uint32_t)h << 16;
                } else {
                    std::memcpy(&u, &all[(off + i) * 4], 4);
                }
                std::memcpy(&(*out)[(size_t)b * kv0 + (size_t)kh * hs + i], &u, 4);
            }
        }
    for (int b = 0; b < B; b++)
        for (int kh = 0; kh < kv0 / hs; kh++)
            std::memset(&all[hipk::kvOff(hipk::KvMap{}, seqLen, kv0 / hs, hs, slot[b], pos[b], kh) * eb],
                        Scratch::kGuardByte, (size_t)hs * eb);
    for (size_t i = 0; i < all.size(); i++)
        DL_CHECK(all[i] == Scratch::kGuardByte, std::string("ops: the launch wrote outside the appended rows of ") + what);
}

void checkRows(const std::vector<float> &v, size_t want, const char *what) {
    DL_CHECK(v.empty() || v.size() == want, std::string("ops: bad size of ") + what);
}

// PRO_RESNORM operands shared by the Q40 ops with a norm prologue: weights tiled at the geometry's
// L, in / residual / norm weights uploaded, xNext (guarded) when there is a residual.
hipk::GemvArgs resnormArgs(Scratch &sc, const std::vector<uint8_t> &blocks, int rows, int n,
                           const std::vector<float> &in, const std::vector<float> &residual,
                           const std::vector<float> &normW, float eps, int B, const Q40Geom &g) {
    DL_CHECK(B == 1 || B == 2 || B == 4, "gemv batch must be 1, 2 or 4");
    DL_CHECK(n % 32 == 0 && in.size() == (size_t)B * n, "gemv input size");
    checkRows(residual, (size_t)B * n, "residual");
    checkRows(normW, (size_t)n, "norm weights");
    const DevQ40 w = uploadQ40(sc, blocks, rows, n, g.lanes);
    hipk::GemvArgs a;
    a.qs = w.qs;
    a.wd = w.d;
    a.rows = rows;
    a.n = n;
    a.lanes = g.lanes;
    a.passes = g.passes;
    a.in = sc.upload(in);
    a.ldIn = n;
    a.addIn = sc.upload(residual);
    // rows of ldIn = n floats back to back: one guard after the last
    a.xNext = residual.empty() ? nullptr : sc.allocGuarded<float>(1, (size_t)B * n, (size_t)B * n + 256, "xNext");
    a.normW = sc.upload(normW);
    a.eps = eps;
    a.act = 1;
    return a;
}

}  // namespace

std::vector<float> gemvQ40(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                           int epi, std::vector<float> *xNext, int lanes, int passes) {
    DL_CHECK(B == 1 || B == 2 || B == 4, "gemv batch must be 1, 2 or 4");
    DL_CHECK(epi == 0 || (epi == 1 && rows % 2 == 0), "gemv epilogue");
    const int ep = epi == 1 ? hipk::EPI_ACT : hipk::EPI_STORE;
    const Q40Geom g = q40Geom(rows, n, B, ep, lanes, passes);
    DL_CHECK(B == 1 || hipk::gemvLdsBytes(n, B, true, g.wgRows, hipk::PRO_RESNORM) <= 64 * 1024,
             "gemv LDS footprint too large for this batch");
    Scratch sc;
    hipk::GemvArgs a = resnormArgs(sc, blocks, rows, n, in, residual, normW, eps, B, g);
    const int outRows = epi == 1 ? rows / 2 : rows;
    a.ldOut = outRows + g.wgRows;
    a.out = sc.allocGuarded<float>(B, outRows, a.ldOut, "the GEMV output");
    hipk::launchGemv(a, B, hipk::PRO_RESNORM, ep, true, sc.s);
    sc.sync();
    sc.checkGuards();
    if (xNext && a.xNext) *xNext = sc.download(a.xNext, (size_t)B * n);
    return sc.downloadRows(a.out, B, outRows, a.ldOut);
}

void gemvQ40SwigluQ80(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                      const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                      int lanes, int passes, std::vector<int8_t> &codes, std::vector<float> &scales) {
    DL_CHECK(rows > 0 && rows % 64 == 0, "gemv SwiGLU -> Q80: rows must be whole 64-row (32 hidden unit) blocks");
    const Q40Geom g = q40Geom(rows, n, B, hipk::EPI_ACT_Q80, lanes, passes);
    Scratch sc;
    hipk::GemvArgs a = resnormArgs(sc, blocks, rows, n, in, residual, normW, eps, B, g);
    const int hidden = rows / 2;
    a.ldOut = hidden + g.wgRows;  // a multiple of 32: the scale pairs are [B][ldOut / 32]
    a.oq = sc.allocGuarded<int8_t>(B, hidden, a.ldOut, "the Q80 codes");
    float *os = sc.allocGuarded<float>(B, (size_t)hidden / 32 * 2, (size_t)a.ldOut / 32 * 2, "the Q80 scales");
    a.os = reinterpret_cast<float2 *>(os);
    hipk::launchGemv(a, B, hipk::PRO_RESNORM, hipk::EPI_ACT_Q80, true, sc.s);
    sc.sync();
    sc.checkGuards();
    codes = sc.downloadRows(a.oq, B, hidden, a.ldOut);
    scales = sc.downloadRows(os, B, (size_t)hidden / 32 * 2, (size_t)a.ldOut / 32 * 2);
}

int gemvQ40Argmax(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                  const std::vector<float> &residual, const std::vector<float> &normW, float eps, int vocabStart,
                  int lanes, int passes, int repeat) {
    DL_CHECK(repeat >= 1 && repeat <= 8, "gemv argmax: 1..8 launches");
    const Q40Geom g = q40Geom(rows, n, 1, hipk::EPI_ARGMAX, lanes, passes);
    Scratch sc;
    hipk::GemvArgs a = resnormArgs(sc, blocks, rows, n, in, residual, normW, eps, 1, g);
    const int grid = (rows + g.wgRows - 1) / g.wgRows;
    a.am.partV = sc.allocGuarded<float>(1, grid, grid + 64, "the argmax partial values");
    a.am.partI = sc.allocGuarded<int>(1, grid, grid + 64, "the argmax partial rows");
    int *ids = sc.allocGuarded<int>(1, repeat, repeat + 16, "the argmax ids");
    a.am.counter = sc.alloc<int>(1);  // zeroed
    a.am.vocabStart = vocabStart;
    for (int i = 0; i < repeat; i++) {
        a.am.ids = ids + i;
        hipk::launchGemv(a, 1, hipk::PRO_RESNORM, hipk::EPI_ARGMAX, true, sc.s);
    }
    sc.sync();
    sc.checkGuards();
    DL_CHECK(sc.download(a.am.counter, 1)[0] == 0, "gemv argmax: the arrival counter did not return to zero");
    const std::vector<int> got = sc.download(ids, repeat);
    for (int i = 1; i < repeat; i++) DL_CHECK(got[i] == got[0], "gemv argmax: repeated launches on the same scratch disagree");
    return got[0];
}

std::vector<float> gemvQ40Q80In(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                                int B, int lanes, int passes) {
    DL_CHECK(B == 1 || B == 2 || B == 4, "gemv batch must be 1, 2 or 4");
    DL_CHECK(n % 32 == 0 && in.size() == (size_t)B * n, "gemv input size");
    const Q40Geom g = q40Geom(rows, n, B, hipk::EPI_STORE, lanes, passes);
    Scratch sc;
    const DevQ40 w = uploadQ40(sc, blocks, rows, n, g.lanes);
    // host Q80 (the reference quantizer) -> int8 codes + (d, sum of codes) per block, as the
    // attention / SwiGLU epilogues hand them to this kernel
    const int nb = n / 32;
    std::vector<BlockQ80> q((size_t)B * nb);
    quantizeQ80(in.data(), q.data(), (u64)B * n);
    std::vector<int8_t> codes((size_t)B * n);
    std::vector<float> scales((size_t)B * nb * 2);
    for (size_t i = 0; i < q.size(); i++) {
        int s = 0;
        for (int j = 0; j < 32; j++) {
            codes[i * 32 + j] = q[i].qs[j];
            s += q[i].qs[j];
        }
        scales[2 * i] = f16ToF32(q[i].d);
        scales[2 * i + 1] = (float)s;
    }
    hipk::GemvArgs a;
    a.qs = w.qs;
    a.wd = w.d;
    a.rows = rows;
    a.n = n;
    a.lanes = g.lanes;
    a.passes = g.passes;
    a.aq = sc.upload(codes);
    a.as = reinterpret_cast<const float2 *>(sc.upload(scales));
    a.ldOut = rows + g.wgRows;
    a.out = sc.allocGuarded<float>(B, rows, a.ldOut, "the GEMV output");
    hipk::launchGemv(a, B, hipk::PRO_GLOBAL, hipk::EPI_STORE, true, sc.s);
    sc.sync();
    sc.checkGuards();
    return sc.downloadRows(a.out, B, rows, a.ldOut);
}

std::vector<float> gemvF32(const std::vector<float> &w, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                           int pro, int epi, int lanes, int passes, std::vector<float> *xNext) {
    DL_CHECK(B == 1 || B == 2 || B == 4, "gemv batch must be 1, 2 or 4");
    DL_CHECK(pro == 0 || pro == 1, "gemv_f32 prologue: 0 global, 1 residual + norm");
    DL_CHECK(epi == 0 || (epi == 1 && rows % 2 == 0), "gemv_f32 epilogue: 0 store, 1 SwiGLU (even rows)");
    DL_CHECK(rows > 0 && n > 0 && n % 8 == 0, "gemv_f32: input width must be a multiple of 8");
    DL_CHECK(w.size() == (size_t)rows * n && in.size() == (size_t)B * n, "gemv_f32 operand sizes");
    DL_CHECK(pro == 1 || (residual.empty() && normW.empty()), "gemv_f32: the global prologue takes no residual or norm");
    // no engine launch pairs them (the F32 w13 GEMV always normalizes), so no instance is compiled
    DL_CHECK(pro == 1 || epi == 0, "gemv_f32: the global prologue has no SwiGLU instance");
    checkRows(residual, (size_t)B * n, "residual");
    checkRows(normW, (size_t)n, "norm weights");
    checkLanes(lanes);
    DL_CHECK(passes >= 0, "gemv passes must be 0 (default) or >= 1");
    const int pr = pro == 1 ? hipk::PRO_RESNORM : hipk::PRO_GLOBAL, ep = epi == 1 ? hipk::EPI_ACT : hipk::EPI_STORE;
    const int L = lanes > 0 ? lanes : hipk::gemvLanesPerRow(n, rows, B, false);
    const int rp = 256 / L * hipk::gemvRowGroup(B, false);
    // the default of the shape's own lane count; a forced one keeps its rule (1..4, grid / 1024)
    const int grid0 = (rows + rp - 1) / rp;
    const int P = passes > 0 ? passes
                             : (lanes > 0 ? std::max(1, std::min(4, grid0 / 1024))
                                          : hipk::gemvDefaultPasses(n, rows, B, false, ep));
    const int wgRows = rp * P;
    DL_CHECK(hipk::gemvLdsBytes(n, B, false, wgRows, pr) <= kLdsLimit, "gemv LDS footprint beyond the device limit");
    Scratch sc;
    hipk::GemvArgs a;
    a.wf = sc.upload(w);
    a.rows = rows;
    a.n = n;
    a.lanes = L;
    a.passes = P;
    a.in = sc.upload(in);
    a.ldIn = n;
    a.addIn = sc.upload(residual);
    a.xNext = residual.empty() ? nullptr : sc.allocGuarded<float>(1, (size_t)B * n, (size_t)B * n + 256, "xNext");
    a.normW = sc.upload(normW);
    a.eps = eps;
    a.act = 1;
    const int outRows = epi == 1 ? rows / 2 : rows;
    a.ldOut = outRows + wgRows;
    a.out = sc.allocGuarded<float>(B, outRows, a.ldOut, "the GEMV output");
    hipk::launchGemv(a, B, pr, ep, false, sc.s);
    sc.sync();
    sc.checkGuards();
    if (xNext && a.xNext) *xNext = sc.download(a.xNext, (size_t)B * n);
    return sc.downloadRows(a.out, B, outRows, a.ldOut);
}

void gemvDefaults(int rows, int n, int B, bool q40, int epi, int &lanes, int &passes) {
    lanes = hipk::gemvLanesPerRow(n, rows, q40 ? 1 : B, q40);
    passes = hipk::gemvDefaultPasses(n, rows, B, q40, epi, q40 ? lanes : 0);
}

void tileQ40Host(const std::vector<uint8_t> &blocks, int rows, int n, int lanes, bool aos, std::vector<uint8_t> &qs,
                 std::vector<uint32_t> &d) {
    DL_CHECK(n > 0 && n % 32 == 0 && rows > 0, "Q40 shape");
    DL_CHECK(lanes == 16 || lanes == 32 || lanes == 64, "tiling lanes must be 16, 32 or 64");
    const size_t nb = (size_t)n / 32;
    DL_CHECK(blocks.size() == (size_t)rows * nb * sizeof(BlockQ40), "Q40 blocks size");
    const hipk::Q40Tiling t = hipk::q40Tiling(rows, n, lanes);
    // preset to a pattern neither writer produces as padding: every byte of the image must be written
    qs.assign(t.qsBytes, 0xEE);
    d.assign(t.dBytes / 4, 0xEEEEEEEEu);
    if (aos) {
        std::vector<const uint8_t *> rowPtr(rows);
        for (int r = 0; r < rows; r++) rowPtr[r] = blocks.data() + (size_t)r * nb * sizeof(BlockQ40);
        hipk::tileQ40AoS(rowPtr.data(), rows, n, lanes, qs.data(), d.data());
        return;
    }
    std::vector<uint8_t> nib((size_t)rows * nb * 16);
    std::vector<uint16_t> sc((size_t)rows * nb);
    const BlockQ40 *b = reinterpret_cast<const BlockQ40 *>(blocks.data());
    for (size_t i = 0; i < (size_t)rows * nb; i++) {
        std::memcpy(&nib[i * 16], b[i].qs, 16);
        sc[i] = b[i].d;
    }
    hipk::tileQ40(nib.data(), sc.data(), rows, n, lanes, qs.data(), d.data());
}

std::vector<float> gemmQ40(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int M,
                           int splits) {
    DL_CHECK(splits == 0 || (splits > 0 && (n / 32) % splits == 0), "gemm splits must divide n / 32");
    DL_CHECK(M >= 1 && M <= 2048, "gemm tokens must be 1..2048");
    DL_CHECK(in.size() == (size_t)M * n, "gemm input size");
    DL_CHECK(hipk::gemmSupported(n), "gemm input width must be a multiple of 32");
    checkRows(residual, (size_t)M * n, "residual");
    checkRows(normW, (size_t)n, "norm weights");
    Scratch sc;
    const DevQ40 w = uploadQ40(sc, blocks, rows, n);
    hipk::GemvArgs nq;
    nq.n = n;
    nq.in = sc.upload(in);
    nq.ldIn = n;
    nq.addIn = sc.upload(residual);
    nq.normW = sc.upload(normW);
    nq.eps = eps;
    // rows past M are read by the last launch (padded to 16/32) and their outputs dropped
    const int rowsPad = (M + hipk::kGemmMaxTokens - 1) / hipk::kGemmMaxTokens * hipk::kGemmMaxTokens;
    _Float16 *xh = sc.alloc<_Float16>((size_t)rowsPad * n);
    hipk::launchNormF16(nq, xh, M, sc.s);
    float *out = sc.alloc<float>((size_t)M * rows);
    size_t part = hipk::gemmPartFloats(rows, n, M);
    if (splits > 0) part = std::max(part, (size_t)splits * ((rows + 127) / 128) * (size_t)rowsPad * 128);
    float *partBuf = part ? sc.alloc<float>(part) : nullptr;
    int *counters = sc.alloc<int>((size_t)hipk::gemmCounterInts(rows, M) + (size_t)(rows + 63) / 64 * (M / 128 + 1) + 1);
    // the engine's chunking: one wide launch, or <= 128 tokens per narrow launch
    const int chunk = hipk::gemmUsesWide(M) ? M : hipk::kGemmMaxTokens;
    for (int c0 = 0; c0 < M; c0 += chunk) {
        const int bc = std::min(chunk, M - c0);
        hipk::GemmArgs g;
        g.e.qs = w.qs;
        g.e.wd = w.d;
        g.e.rows = rows;
        g.e.n = n;
        g.e.lanes = w.lanes;
        g.e.out = out + (size_t)c0 * rows;
        g.e.ldOut = rows;
        g.x = xh + (size_t)c0 * n;
        g.M = bc;
        g.splits = splits > 0 ? splits : hipk::gemmSplits(rows, n, bc, w.lanes);
        g.part = partBuf;
        g.counters = counters;
        hipk::launchGemmQ40(g, hipk::EPI_STORE, sc.s);
    }
    sc.sync();
    return sc.download(out, (size_t)M * rows);
}

// Batched F32-weight GEMM (K5): RMS norm -> f16 activations -> gemmF32Kernel, EPI_STORE.
std::vector<float> gemmF32(const std::vector<float> &w, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &normW, float eps, int M) {
    DL_CHECK(M >= 1 && M <= 256, "gemm tokens must be 1..256");
    DL_CHECK(w.size() == (size_t)rows * n && in.size() == (size_t)M * n, "gemm operand sizes");
    DL_CHECK(hipk::gemmSupported(n), "gemm input width must be a multiple of 32");
    checkRows(normW, (size_t)n, "norm weights");
    Scratch sc;
    hipk::GemvArgs nq;
    nq.n = n;
    nq.in = sc.upload(in);
    nq.ldIn = n;
    nq.normW = sc.upload(normW);
    nq.eps = eps;
    const int rowsPad = (M + hipk::kGemmF32MaxTokens - 1) / hipk::kGemmF32MaxTokens * hipk::kGemmF32MaxTokens;
    _Float16 *xh = sc.alloc<_Float16>((size_t)rowsPad * n);
    hipk::launchNormF16(nq, xh, M, sc.s);
    const float *wd = sc.upload(w);
    float *out = sc.alloc<float>((size_t)M * rows);
    const size_t part = hipk::gemmPartFloats(rows, n, M);
    float *partBuf = part ? sc.alloc<float>(part) : nullptr;
    int *counters = sc.alloc<int>((size_t)(rows + 63) / 64 + 1);
    for (int c0 = 0; c0 < M; c0 += hipk::kGemmF32MaxTokens) {
        const int bc = std::min(hipk::kGemmF32MaxTokens, M - c0);
        hipk::GemmArgs g;
        g.e.wf = wd;
        g.e.rows = rows;
        g.e.n = n;
        g.e.out = out + (size_t)c0 * rows;
        g.e.ldOut = rows;
        g.x = xh + (size_t)c0 * n;
        g.M = bc;
        g.splits = hipk::gemmSplits(rows, n, bc);
        g.part = partBuf;
        g.counters = counters;
        hipk::launchGemmF32(g, hipk::EPI_STORE, sc.s);
    }
    sc.sync();
    return sc.download(out, (size_t)M * rows);
}

std::vector<GemmLaunch> gemmBatchedPlan(const GemmBatchedArgs &a) {
    const bool q40 = a.wf.empty();
    const int rows = a.rows, n = a.n, M = a.M;
    DL_CHECK(rows > 0 && n > 0 && hipk::gemmSupported(n), "gemm input width must be a multiple of 32");
    DL_CHECK(M >= 1 && M <= 2048, "gemm tokens must be 1..2048");
    if (q40) {
        checkLanes(a.lanes);
        DL_CHECK(a.blocks.size() == (size_t)rows * (n / 32) * sizeof(BlockQ40), "Q40 blocks size");
    } else {
        DL_CHECK(a.blocks.empty() && a.wf.size() == (size_t)rows * n, "gemm F32 weights size");
    }
    DL_CHECK(a.in.size() == (size_t)M * n, "gemm input size");
    if (a.input == GEMM_IN_NORM) {
        checkRows(a.residual, (size_t)M * n, "residual");
        checkRows(a.normW, (size_t)n, "norm weights");
    } else {
        DL_CHECK(a.input == GEMM_IN_F16 || a.input == GEMM_IN_PRENORM, "gemm input mode");
        DL_CHECK(a.residual.empty() && a.normW.empty(), "gemm: f16 / prenorm rows take no residual or norm weights");
    }
    const bool ssUsed = a.input == GEMM_IN_PRENORM || a.epi == hipk::EPI_RES;
    DL_CHECK(!ssUsed || a.ldSS >= M, "gemm ldSS must be at least the token count");
    if (a.input == GEMM_IN_PRENORM)
        DL_CHECK(a.ssTiles >= 1 && a.ss.size() == (size_t)a.ssTiles * a.ldSS, "gemm prenorm sums of squares: [ssTiles][ldSS]");
    switch (a.epi) {
        case hipk::EPI_STORE: break;
        case hipk::EPI_ACT_F16: DL_CHECK(rows % 2 == 0, "gemm SwiGLU: rows are (w1, w3) pairs"); break;
        case hipk::EPI_RES:
            DL_CHECK(rows % 2 == 0, "gemm EPI_RES: the epilogue stores whole row pairs (even rows)");
            DL_CHECK(a.resIn.size() == (size_t)M * rows && a.resW.size() == (size_t)rows, "gemm EPI_RES operand sizes");
            break;
        case hipk::EPI_QKV:
            DL_CHECK((a.hs == 64 || a.hs == 128) && a.q0 > 0 && a.kv0 > 0 && a.q0 % a.hs == 0 && a.kv0 % a.hs == 0 &&
                         rows == a.q0 + 2 * a.kv0, "qkv head layout");
            DL_CHECK(a.seqLen > 0 && a.nSlots > 0 && a.rope.size() == (size_t)a.seqLen * a.hs &&
                         a.pos.size() == (size_t)M && a.slot.size() == (size_t)M, "qkv operand sizes");
            for (int t = 0; t < M; t++)
                DL_CHECK(a.pos[t] >= 0 && a.pos[t] < a.seqLen && a.slot[t] >= 0 && a.slot[t] < a.nSlots,
                         "qkv position / slot out of range");
            break;
        default: throw Error("gemm epilogue: the engine launches only store, SwiGLU -> f16, residual and QKV on a GEMM");
    }
    DL_CHECK(a.splits >= 0 && a.chunk >= 0 && (a.fixed == 0 || a.fixed == 1), "gemm launch controls");
    const int L = q40 ? (a.lanes > 0 ? a.lanes : hipk::gemvLanesPerRow(n, rows, 1, true)) : 0;
    const int chunk = a.chunk > 0 ? a.chunk : hipk::gemmChunkTokens(n, M, q40, a.fixed != 0);
    const int tiles = (rows + 63) / 64;
    std::vector<GemmLaunch> plan;
    for (int c0 = 0; c0 < M; c0 += chunk) {
        GemmLaunch l;
        l.c0 = c0;
        l.M = std::min(chunk, M - c0);
        l.splits = a.splits > 0 ? a.splits : a.fixed ? hipk::gemmSplits(rows, n, 16, 0) : hipk::gemmSplits(rows, n, l.M, L);
        DL_CHECK((n / 32) % l.splits == 0, "gemm splits must divide n / 32");
        l.grid = tiles * l.splits;
        if (q40) {
            l.kernel = hipk::gemmKernelFor(n, l.M, L, l.splits, a.fixed != 0);
            if (l.kernel == hipk::GEMM_WIDE) {
                DL_CHECK(hipk::gemmWideAccepts(n, l.splits), "wide gemm: bad K split (whole two-block stages per split)");
                l.grid = (rows + 127) / 128 * ((l.M + 127) / 128) * l.splits;
            } else {
                DL_CHECK(l.M <= hipk::kGemmMaxTokens, "gemm: more than 128 tokens per narrow launch");
            }
        } else {
            l.kernel = 3;
            DL_CHECK(l.M <= hipk::kGemmF32MaxTokens, "gemm: more than 64 tokens per F32 launch");
        }
        plan.push_back(l);
    }
    return plan;
}

int gemmSplitsFor(int rows, int n, int M, int lanes) {
    DL_CHECK(rows > 0 && n > 0 && n % 32 == 0 && M >= 1, "gemm shape");
    return hipk::gemmSplits(rows, n, M, lanes);
}

GemmBatchedResult gemmBatched(const GemmBatchedArgs &a) {
    const std::vector<GemmLaunch> plan = gemmBatchedPlan(a);  // refusals: before any device work
    const bool q40 = a.wf.empty();
    const int rows = a.rows, n = a.n, M = a.M, epi = a.epi;
    Scratch sc;
    DevQ40 w;
    const float *wf = nullptr;
    if (q40)
        w = uploadQ40(sc, a.blocks, rows, n, a.lanes);
    else
        wf = sc.upload(a.wf);
    // activations: rows past a launch's tokens are read by design (token tiles of 16..128), zeroed here
    _Float16 *xh = sc.alloc<_Float16>((size_t)(M + 128) * n);
    hipk::GemvArgs nq;
    if (a.input == GEMM_IN_NORM) {
        nq.n = n;
        nq.in = sc.upload(a.in);
        nq.ldIn = n;
        nq.addIn = sc.upload(a.residual);
        nq.normW = sc.upload(a.normW);
        nq.eps = a.eps;
    } else {
        std::vector<uint16_t> h(a.in.size());
        for (size_t i = 0; i < h.size(); i++) h[i] = f32ToF16(a.in[i]);
        DL_HIP(hipMemcpyAsync(xh, h.data(), h.size() * 2, hipMemcpyHostToDevice, sc.s));
        DL_HIP(hipStreamSynchronize(sc.s));
    }
    const float *ssIn = a.input == GEMM_IN_PRENORM ? sc.upload(a.ss) : nullptr;
    // outputs: a guard after each token row's valid columns and whole guard rows after the last token
    // (as many as the last token tile's padding, so a store of any dropped token lands in one)
    const int outCols = epi == hipk::EPI_ACT_F16 ? rows / 2 : epi == hipk::EPI_QKV ? a.q0 : rows;
    const int ldOut = outCols + 128;
    const size_t tail = (size_t)(M + 127) / 128 * 128 - M + 16;
    float *out = nullptr, *ssOut = nullptr;
    uint16_t *outH = nullptr, *resX = nullptr;
    const float *resIn = nullptr, *resW = nullptr;
    const int ssRows = (rows + 63) / 64;
    if (epi == hipk::EPI_ACT_F16)
        outH = sc.allocGuardedTail<uint16_t>(M, outCols, ldOut, tail, "the f16 SwiGLU rows");
    else
        out = sc.allocGuardedTail<float>(M, outCols, ldOut, tail, epi == hipk::EPI_RES ? "resOut" : "the GEMM output");
    if (epi == hipk::EPI_RES) {
        resX = sc.allocGuardedTail<uint16_t>(M, rows, ldOut, tail, "resX");
        ssOut = sc.allocGuardedTail<float>(ssRows, M, a.ldSS, 2, "ssOut");
        std::vector<float> padded((size_t)M * ldOut, 0.f);  // resIn shares the outputs' row stride
        for (int t = 0; t < M; t++) std::copy(a.resIn.begin() + (size_t)t * rows, a.resIn.begin() + (size_t)(t + 1) * rows, padded.begin() + (size_t)t * ldOut);
        resIn = sc.upload(padded);
        resW = sc.upload(a.resW);
    }
    size_t cacheElems = 0;
    uint8_t *kc = nullptr, *vc = nullptr;
    const float2 *rope = nullptr;
    const int *pos = nullptr, *slot = nullptr;
    if (epi == hipk::EPI_QKV) {
        // the caches are preset to the guard pattern as a whole (plus a guard after the last slot):
        // only the appended rows may change
        cacheElems = (size_t)a.nSlots * a.seqLen * a.kv0;
        const size_t eb = a.kvBf16 ? 2 : 4, cacheGuard = (size_t)128 * a.seqLen;
        kc = sc.allocGuarded<uint8_t>(1, cacheElems * eb, (cacheElems + cacheGuard) * eb, "the K cache");
        vc = sc.allocGuarded<uint8_t>(1, cacheElems * eb, (cacheElems + cacheGuard) * eb, "the V cache");
        rope = reinterpret_cast<const float2 *>(sc.upload(a.rope));
        pos = sc.upload(a.pos);
        slot = sc.upload(a.slot);
    }
    size_t part = 0, counters = (size_t)ssRows;
    for (const GemmLaunch &l : plan) {
        if (l.kernel == hipk::GEMM_WIDE) {
            const size_t wt = (size_t)((rows + 127) / 128) * ((l.M + 127) / 128);
            part = std::max(part, l.splits * wt * 128 * 128);
            counters = std::max(counters, wt);
        } else {
            part = std::max(part, (size_t)l.splits * ssRows * hipk::gemmTokenPad(l.M) * 64);
        }
    }
    float *partBuf = sc.alloc<float>(part + 4);
    int *cnt = sc.alloc<int>(counters + 1);  // zeroed
    for (const GemmLaunch &l : plan) {
        const int c0 = l.c0;
        hipk::GemmArgs g;
        hipk::GemvArgs &e = g.e;
        e.qs = w.qs;
        e.wd = w.d;
        e.wf = wf;
        e.rows = rows;
        e.n = n;
        e.lanes = w.lanes;
        e.eps = a.eps;
        if (a.input == GEMM_IN_NORM) {  // the engine normalizes each chunk into the head of its f16 buffer
            hipk::GemvArgs nc = nq;
            nc.in = nq.in + (size_t)c0 * n;
            nc.addIn = nq.addIn ? nq.addIn + (size_t)c0 * n : nullptr;
            hipk::launchNormF16(nc, xh, l.M, sc.s);
            g.x = xh;
        } else {
            g.x = xh + (size_t)c0 * n;
        }
        if (ssIn) {
            g.ssIn = ssIn + c0;
            g.ssTiles = a.ssTiles;
            g.ldSS = a.ldSS;
        }
        e.out = out ? out + (size_t)c0 * ldOut : nullptr;
        g.outH = outH ? reinterpret_cast<_Float16 *>(outH) + (size_t)c0 * ldOut : nullptr;
        e.ldOut = ldOut;
        e.act = 1;
        if (epi == hipk::EPI_QKV) {
            e.q0 = a.q0;
            e.kv0 = a.kv0;
            e.hs = a.hs;
            e.seqLen = a.seqLen;
            e.rope = rope;
            e.pos = pos + c0;
            e.slot = slot + c0;
            e.kcache = kc;
            e.vcache = vc;
            e.kvBf16 = a.kvBf16 ? 1 : 0;
        }
        if (epi == hipk::EPI_RES) {
            g.resIn = resIn + (size_t)c0 * ldOut;
            g.resOut = out + (size_t)c0 * ldOut;
            e.out = nullptr;
            g.resW = resW;
            g.resX = reinterpret_cast<_Float16 *>(resX) + (size_t)c0 * ldOut;
            g.ssOut = ssOut + c0;
            g.ldSS = a.ldSS;
        }
        g.M = l.M;
        g.splits = l.splits;
        g.fixed = a.fixed;
        g.part = partBuf;
        g.counters = cnt;
        if (q40)
            hipk::launchGemmQ40(g, epi, sc.s);
        else
            hipk::launchGemmF32(g, epi, sc.s);
    }
    sc.sync();
    sc.checkGuards();
    GemmBatchedResult r;
    r.launches = plan;
    auto widen = [](const std::vector<uint16_t> &h) {
        std::vector<float> f(h.size());
        for (size_t i = 0; i < h.size(); i++) f[i] = f16ToF32(h[i]);
        return f;
    };
    if (outH)
        r.out = widen(sc.downloadRows(outH, M, outCols, ldOut));
    else
        r.out = sc.downloadRows(out, M, outCols, ldOut);
    if (epi == hipk::EPI_RES) {
        r.resX = widen(sc.downloadRows(resX, M, rows, ldOut));
        r.ssOut = sc.download(ssOut, (size_t)ssRows * a.ldSS);
    }
    if (epi == hipk::EPI_QKV) {
        appendedRows(sc, kc, cacheElems, a.seqLen, a.kv0, a.hs, a.pos, a.slot, a.kvBf16, "the K cache", &r.k);
        appendedRows(sc, vc, cacheElems, a.seqLen, a.kv0, a.hs, a.pos, a.slot, a.kvBf16, "the V cache", &r.v);
    }
    return r;
}

std::vector<float> qkvRope(const std::vector<uint8_t> &blocks, int q0, int kv0, int hs, int n,
                           const std::vector<float> &in, const std::vector<float> &normW, float eps,
                           const std::vector<float> &rope, int seqLen, const std::vector<int> &pos, bool kvBf16,
                           std::vector<float> *kOut, std::vector<float> *vOut, int lanes, int passes) {
    const int B = (int)pos.size(), rows = q0 + 2 * kv0;
    DL_CHECK(B == 1 || B == 2 || B == 4, "qkv batch must be 1, 2 or 4");
    DL_CHECK(hs % 2 == 0 && hs <= 128 && q0 % hs == 0 && kv0 % hs == 0, "qkv head layout");
    DL_CHECK(in.size() == (size_t)B * n && rope.size() == (size_t)seqLen * hs, "qkv operand sizes");
    checkRows(normW, (size_t)n, "norm weights");
    for (int p : pos) DL_CHECK(p >= 0 && p < seqLen, "qkv position out of range");
    const Q40Geom g = q40Geom(rows, n, B, hipk::EPI_QKV, lanes, passes);
    Scratch sc;
    const DevQ40 w = uploadQ40(sc, blocks, rows, n, g.lanes);
    std::vector<int> slots(B);
    for (int b = 0; b < B; b++) slots[b] = b;
    // the caches are preset to the guard pattern as a whole (plus a guard after the last slot):
    // only the B appended rows may change
    const size_t cacheElems = (size_t)B * seqLen * kv0, cacheGuard = (size_t)g.wgRows * seqLen;
    const size_t eb = kvBf16 ? 2 : 4;
    uint8_t *kc = sc.allocGuarded<uint8_t>(1, cacheElems * eb, (cacheElems + cacheGuard) * eb, "the K cache");
    uint8_t *vc = sc.allocGuarded<uint8_t>(1, cacheElems * eb, (cacheElems + cacheGuard) * eb, "the V cache");
    hipk::GemvArgs a;
    a.qs = w.qs;
    a.wd = w.d;
    a.rows = rows;
    a.n = n;
    a.lanes = g.lanes;
    a.passes = g.passes;
    a.in = sc.upload(in);
    a.ldIn = n;
    a.normW = sc.upload(normW);
    a.eps = eps;
    a.ldOut = q0 + g.wgRows;
    a.out = sc.allocGuarded<float>(B, q0, a.ldOut, "the rotated queries");
    a.q0 = q0;
    a.kv0 = kv0;
    a.hs = hs;
    a.seqLen = seqLen;
    a.rope = reinterpret_cast<const float2 *>(sc.upload(rope));
    a.pos = sc.upload(pos);
    a.slot = sc.upload(slots);
    a.kcache = kc;
    a.vcache = vc;
    a.kvBf16 = kvBf16 ? 1 : 0;
    hipk::launchGemv(a, B, hipk::PRO_RESNORM, hipk::EPI_QKV, true, sc.s);
    sc.sync();
    sc.checkGuards();
    std::vector<float> k, v;
    appendedRows(sc, kc, cacheElems, seqLen, kv0, hs, pos, slots, kvBf16, "the K cache", &k);
    appendedRows(sc, vc, cacheElems, seqLen, kv0, hs, pos, slots, kvBf16, "the V cache", &v);
    if (kOut) *kOut = k;
    if (vOut) *vOut = v;
    return sc.downloadRows(a.out, B, q0, a.ldOut);
}

std::vector<float> attention(const std::vector<float> &q, const std::vector<float> &k, const std::vector<float> &v,
                             int nSlots, int seqLen, int nHeads0, int kvMul, int hs, const std::vector<int> &pos,
                             const std::vector<int> &slot, bool kvBf16, int impl) {
    const int B = (int)pos.size();
    DL_CHECK(B >= 1 && slot.size() == pos.size(), "attention rows");
    if (impl == 1) {
        DL_CHECK(hipk::attnPrefillSupported(hs, kvMul, kvBf16), "prefill attention: head size 64 / 128, power-of-two GQA group");
        const int rpb = hipk::attnPrefillRowsPerBlock(kvMul);
        for (int b = 0; b < B; b++) DL_CHECK(slot[b] == slot[b - b % rpb], "prefill row blocks must share a slot");
    }
    DL_CHECK(kvMul >= 1 && nHeads0 % kvMul == 0 && (hs == 64 || hs == 128), "attention head layout");
    const int q0 = nHeads0 * hs, kv0 = nHeads0 / kvMul * hs;
    const size_t cacheElems = (size_t)nSlots * seqLen * kv0;
    DL_CHECK(q.size() == (size_t)B * q0 && k.size() == cacheElems && v.size() == cacheElems, "attention sizes");
    for (int b = 0; b < B; b++)
        DL_CHECK(pos[b] >= 0 && pos[b] < seqLen && slot[b] >= 0 && slot[b] < nSlots, "attention row out of range");
    Scratch sc;
    auto cache = [&](const std::vector<float> &xs) -> void * {
        // the caller's [slot][seqLen][kv0] rows -> the engine's head-major [slot][nKv][seqLen][hs]
        const int nKv = kv0 / hs;
        std::vector<float> x(xs.size());
        for (int sl = 0; sl < nSlots; sl++)
            for (int p = 0; p < seqLen; p++)
                for (int kh = 0; kh < nKv; kh++)
                    std::memcpy(&x[hipk::kvOff(hipk::KvMap{}, seqLen, nKv, hs, sl, p, kh)],
                                &xs[((size_t)sl * seqLen + p) * kv0 + (size_t)kh * hs], hs * sizeof(float));
        if (!kvBf16) return sc.upload(x);
        std::vector<uint16_t> h(x.size());
        for (size_t i = 0; i < x.size(); i++) {  // round to nearest even, as the QKV epilogue stores
            uint32_t u;
            std::memcpy(&u, &x[i], 4);
            h[i] = (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
        }
        return sc.upload(h);
    };
    hipk::AttnArgs a;
    a.q = sc.upload(q);
    a.ldq = q0;
    a.kcache = cache(k);
    a.vcache = cache(v);
    a.pos = sc.upload(pos);
    a.slot = sc.upload(slot);
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
    a.out = sc.alloc<float>((size_t)B * q0);
    a.ldOut = q0;
    a.kvBf16 = kvBf16 ? 1 : 0;
    a.counters = sc.alloc<int>((size_t)B * nHeads0);
    DL_HIP(hipMemsetAsync(a.counters, 0, sizeof(int) * (size_t)B * nHeads0, sc.s));
    if (impl == 1)
        hipk::launchAttentionPrefill(a, B, sc.s);
    else if (impl == 2)
        hipk::launchAttentionValu(a, B, sc.s);
    else if (impl == 3) {
        DL_CHECK(hipk::attnMfmaSupported(a), "MFMA decode attention: bf16 cache, head size 128, kvMul 1/2/4/8");
        hipk::launchAttentionMfma(a, B, sc.s);
    } else
        hipk::launchAttention(a, B, sc.s);
    sc.sync();
    return sc.download(a.out, (size_t)B * q0);
}

namespace {

// The scalar half of the engine's attnArgs (engine_forward.cpp) for an AttnLaunchArgs call: every
// field the launchers' predicates read. The table pointer is a non-null placeholder for paged
// calls (the predicates only test it); attentionLaunch replaces it with the device table.
struct AttnGeom {
    hipk::AttnArgs a;
    int B = 0, q0 = 0, kv0 = 0, nKv = 0, ldq = 0, ldOut = 0, pagesPerSlot = 0, pageShift = 0;
    bool prefill = false;
};
const int kAttnTablePlaceholder = 0;

AttnGeom attnGeom(const AttnLaunchArgs &l) {
    AttnGeom g;
    const int B = g.B = (int)l.pos.size();
    DL_CHECK(B >= 1 && l.slot.size() == l.pos.size(), "attention rows");
    DL_CHECK(l.kvMul >= 1 && l.nHeads0 >= 1 && l.nHeads0 % l.kvMul == 0 && (l.hs == 64 || l.hs == 128), "attention head layout");
    DL_CHECK(l.nSlots >= 1 && l.seqLen >= 1, "attention cache shape");
    g.q0 = l.nHeads0 * l.hs;
    g.nKv = l.nHeads0 / l.kvMul;
    g.kv0 = g.nKv * l.hs;
    g.ldq = l.ldq > 0 ? l.ldq : g.q0;
    g.ldOut = l.ldOut > 0 ? l.ldOut : g.q0;
    DL_CHECK(g.ldq >= g.q0 && g.ldq % 4 == 0, "attention ldq: at least q0, whole float4 loads");
    DL_CHECK(g.ldOut >= g.q0 && g.ldOut % 32 == 0, "attention ldOut: at least q0, whole Q80 blocks");
    const size_t cacheElems = (size_t)l.nSlots * l.seqLen * g.kv0;
    DL_CHECK(l.q.size() == (size_t)B * g.ldq && l.k.size() == cacheElems && l.v.size() == cacheElems, "attention sizes");
    for (int b = 0; b < B; b++)
        DL_CHECK(l.pos[b] >= 0 && l.pos[b] < l.seqLen && l.slot[b] >= 0 && l.slot[b] < l.nSlots, "attention row out of range");
    DL_CHECK(l.kernel >= ATTN_AUTO && l.kernel <= ATTN_PREFILL && (l.mode == ATTN_DECODE || l.mode == ATTN_PREFILL_ROWS),
             "attention kernel / mode");
    g.prefill = l.mode == ATTN_PREFILL_ROWS;
    DL_CHECK(g.prefill ? (l.kernel == ATTN_AUTO || l.kernel == ATTN_PREFILL) : l.kernel != ATTN_PREFILL,
             "attention: the prefill kernels run prefill rows, the decode kernels decode rows");
    DL_CHECK(l.headGroup == 0 || l.headGroup == 1 || l.headGroup == 2 || l.headGroup == 4 || l.headGroup == 8,
             "attention headGroup must be 0 (the launcher's pick), 1, 2, 4 or 8");
    DL_CHECK(l.splitGrid >= 0 && l.splitGrid <= 128, "attention splitGrid must be 0 (the engine's rule) or 1..128");
    DL_CHECK(l.out == ATTN_OUT_F32 || l.out == ATTN_OUT_F16 || l.out == ATTN_OUT_Q80, "attention output format");
    DL_CHECK(l.repeat >= 1, "attention repeat must be at least 1");
    DL_CHECK(l.warmPos.empty() || l.warmPos.size() == l.pos.size(), "attention warm positions: one per row");
    for (int p : l.warmPos) DL_CHECK(p >= 0 && p < l.seqLen, "attention warm position out of range");
    DL_CHECK(!(g.prefill && l.out == ATTN_OUT_Q80), "attention: the prefill kernels ignore outQ (no Q80 output)");
    DL_CHECK((l.poisonK.empty() || l.poisonK.size() == (size_t)g.kv0) && (l.poisonV.empty() || l.poisonV.size() == (size_t)g.kv0),
             "attention poison rows: [kv0]");
    hipk::AttnArgs &a = g.a;
    if (l.pageSize) {
        DL_CHECK(l.pageSize >= 32 && (l.pageSize & (l.pageSize - 1)) == 0, "attention pageSize must be a power of two >= 32");
        while ((1 << g.pageShift) < l.pageSize) g.pageShift++;
        g.pagesPerSlot = (l.seqLen + l.pageSize - 1) / l.pageSize;
        const int nPages = l.nSlots * g.pagesPerSlot;
        DL_CHECK(l.pageOf.size() == (size_t)nPages, "attention pageOf: [nSlots][ceil(seqLen / pageSize)]");
        for (int p : l.pageOf) DL_CHECK(p >= -1 && p < nPages, "attention pageOf: -1 or a pool page below nSlots * pagesPerSlot");
        a.kvMap.table = &kAttnTablePlaceholder;
        a.kvMap.pageShift = g.pageShift;
        a.kvMap.pagesPerSlot = g.pagesPerSlot;
    } else {
        DL_CHECK(l.pageOf.empty(), "attention pageOf needs a pageSize");
    }
    a.ldq = g.ldq;
    a.nHeads0 = l.nHeads0;
    a.kvMul = l.kvMul;
    a.hs = l.hs;
    a.kv0 = g.kv0;
    a.seqLen = l.seqLen;
    a.chunkMin = hipk::attnChunkMin();
    a.shortLen = l.single ? hipk::kAttnShortLen : 0;
    if (l.splitGrid > 0) {
        a.splitGrid = l.splitGrid;
        a.chunkMax = hipk::attnChunkMax(l.seqLen, a.splitGrid);
    } else {
        a.splitGrid = hipk::attnSplitGrid(l.seqLen, l.single);
        a.chunkMax = hipk::attnChunkMax(l.seqLen, hipk::attnSplitGrid(l.seqLen, false));
    }
    a.ldOut = g.ldOut;
    a.kvBf16 = l.kvBf16 ? 1 : 0;
    a.mfma = l.kernel == ATTN_MFMA ? 1 : l.kernel == ATTN_VALU ? 0 : -1;
    a.headGroup = l.headGroup;
    return g;
}

}  // namespace

AttnLaunchPlan attentionPlan(const AttnLaunchArgs &l) {
    const AttnGeom g = attnGeom(l);
    const hipk::AttnArgs &a = g.a;
    AttnLaunchPlan p;
    p.splitGrid = a.splitGrid;
    p.chunkMax = a.chunkMax;
    p.shortLen = a.shortLen;
    const std::string hsS = std::to_string(a.hs), kmS = std::to_string(a.kvMul);
    if (g.prefill) {
        if (const char *why = hipk::attnPrefillRefusal(a)) throw Error(why);
        const int rpb = hipk::attnPrefillRowsPerBlock(a.kvMul);
        for (int b = 0; b < g.B; b++) DL_CHECK(l.slot[b] == l.slot[b - b % rpb], "prefill row blocks must share a slot");
        p.kernel = hipk::attnPrefillDmaSupported(a) ? "attnPrefillDmaKernel<" + kmS + ">"
                   : a.kvBf16                       ? "attnPrefillKernel<" + hsS + ">"
                                                    : "attnPrefillF32Kernel<" + hsS + ">";
        p.grid[0] = g.nKv * ((g.B + rpb - 1) / rpb);
        p.grid[1] = a.splitGrid;
        p.grid[2] = 1;
        const int chunkKeys = hipk::attnPrefillChunkKeys(a, p.grid[0]);
        for (int b0 = 0; b0 < g.B; b0 += rpb) {
            int maxLen = 0, ns, ch;
            for (int b = b0; b < std::min(g.B, b0 + rpb); b++) maxLen = std::max(maxLen, l.pos[b] + 1);
            hipk::attnPrefillSplit(maxLen, a.splitGrid, a.hs, chunkKeys, ns, ch);
            p.nSplit.push_back(ns);
            p.ch.push_back(ch);
        }
        return p;
    }
    bool mfma;
    if (l.kernel == ATTN_MFMA) {
        DL_CHECK(hipk::attnMfmaSupported(a), "MFMA decode attention: bf16 cache, head size 128, kvMul 1/2/4/8");
        mfma = true;
    } else {
        mfma = l.kernel == ATTN_AUTO && hipk::attnUsesMfma(a);
    }
    if (mfma) {
        if (const char *why = hipk::attnMfmaRefusal(a)) throw Error(why);
        p.kernel = "attnDecodeMfmaKernel<" + kmS + ">";
        p.grid[0] = g.nKv;
    } else {
        p.hg = hipk::attnValuHeadGroup(a, g.B);
        p.kernel = "attnKernel<" + std::to_string(p.hg) + "," + hsS + (a.kvBf16 ? ",bf16>" : ",f32>");
        p.grid[0] = a.nHeads0 / p.hg;
    }
    p.grid[1] = a.splitGrid;
    p.grid[2] = g.B;
    for (int b = 0; b < g.B; b++) {
        int ns, ch;
        hipk::attnSplit(l.pos[b] + 1, a.splitGrid, ns, ch, a.chunkMin, a.shortLen);
        p.nSplit.push_back(ns);
        p.ch.push_back(ch);
    }
    return p;
}

AttnLaunchResult attentionLaunch(const AttnLaunchArgs &l) {
    AttnLaunchResult res;
    res.plan = attentionPlan(l);  // refusals: before any device work
    AttnGeom g = attnGeom(l);
    hipk::AttnArgs &a = g.a;
    const int B = g.B, q0 = g.q0, kv0 = g.kv0, nKv = g.nKv, hs = l.hs, seqLen = l.seqLen;
    Scratch sc;
    // caches: the caller's [slot][seqLen][kv0] rows -> the engine's head-major layout through kvOff,
    // contiguous [slot][nKv][seqLen][hs] or a pool [page][nKv][pageSize][hs] (+ the poison page)
    hipk::KvMap hostMap;  // contiguous: no table
    size_t poolElems = (size_t)l.nSlots * seqLen * kv0;
    const int nPages = l.nSlots * g.pagesPerSlot;
    std::vector<int> table;
    if (l.pageSize) {
        table = l.pageOf;
        for (int &t : table)
            if (t < 0) t = nPages;  // the poison page
        hostMap.table = table.data();
        hostMap.pageShift = g.pageShift;
        hostMap.pagesPerSlot = g.pagesPerSlot;
        poolElems = (size_t)(nPages + 1) * kv0 * l.pageSize;
    }
    auto cache = [&](const std::vector<float> &xs, const std::vector<float> &poison) -> void * {
        std::vector<float> x(poolElems, 0.f);
        if (l.pageSize) {  // every page holds the poison row until a table entry claims it
            for (int pg = 0; pg <= nPages; pg++)
                for (int kh = 0; kh < nKv; kh++)
                    for (int p = 0; p < l.pageSize; p++)
                        for (int d = 0; d < hs; d++)
                            x[(((size_t)pg * nKv + kh) * l.pageSize + p) * hs + d] = poison.empty() ? 0.f : poison[(size_t)kh * hs + d];
        }
        for (int sl = 0; sl < l.nSlots; sl++)
            for (int p = 0; p < seqLen; p++) {
                if (l.pageSize && l.pageOf[(size_t)sl * g.pagesPerSlot + (p >> g.pageShift)] < 0) continue;
                for (int kh = 0; kh < nKv; kh++)
                    std::memcpy(&x[hipk::kvOff(hostMap, seqLen, nKv, hs, sl, p, kh)],
                                &xs[((size_t)sl * seqLen + p) * kv0 + (size_t)kh * hs], hs * sizeof(float));
            }
        if (!l.kvBf16) return sc.upload(x);
        std::vector<uint16_t> h(x.size());
        for (size_t i = 0; i < x.size(); i++) {  // round to nearest even, as the QKV epilogue stores
            uint32_t u;
            std::memcpy(&u, &x[i], 4);
            h[i] = (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
        }
        return sc.upload(h);
    };
    a.q = sc.upload(l.q);
    a.kcache = cache(l.k, l.poisonK);
    a.vcache = cache(l.v, l.poisonV);
    if (l.pageSize) a.kvMap.table = sc.upload(table);
    a.pos = sc.upload(l.pos);
    a.slot = sc.upload(l.slot);
    // scratch of the engine's sizes (engine_load.cpp), each followed by a guard
    const size_t nPartO = (size_t)B * l.nHeads0 * a.splitGrid * hs, nPartML = (size_t)B * l.nHeads0 * a.splitGrid * 2;
    const size_t nCnt = (size_t)B * l.nHeads0, guard = 256;
    a.partO = sc.allocGuarded<float>(1, nPartO, nPartO + guard, "partO");
    a.partML = sc.allocGuarded<float>(1, nPartML, nPartML + guard, "partML");
    a.counters = sc.allocGuarded<int>(1, nCnt, nCnt + guard, "the arrival counters");
    DL_HIP(hipMemsetAsync(a.counters, 0, nCnt * sizeof(int), sc.s));
    // the output: a guard after each row's q0 valid elements (ldOut > q0) and two guard rows after the last
    const size_t ldO = g.ldOut, ldS = ldO / 32, tail = 2;
    void *outBuf = nullptr;
    size_t outBytes = 0, sBytes = 0;
    if (l.out == ATTN_OUT_Q80) {
        a.outQ = sc.allocGuardedTail<int8_t>(B, q0, ldO, tail, "the Q80 codes");
        a.outS = reinterpret_cast<float2 *>(sc.allocGuardedTail<float>(B, (size_t)q0 / 32 * 2, ldS * 2, tail, "the Q80 scales"));
        outBuf = a.outQ;
        outBytes = (B + tail) * ldO;
        sBytes = (B + tail) * ldS * 2 * sizeof(float);
    } else if (l.out == ATTN_OUT_F16) {
        a.outH = reinterpret_cast<_Float16 *>(sc.allocGuardedTail<uint16_t>(B, q0, ldO, tail, "the f16 output"));
        outBuf = a.outH;
        outBytes = (B + tail) * ldO * 2;
    } else {
        a.out = sc.allocGuardedTail<float>(B, q0, ldO, tail, "the attention output");
        outBuf = a.out;
        outBytes = (B + tail) * ldO * 4;
    }
    auto run = [&] {
        if (g.prefill)
            hipk::launchAttentionPrefill(a, B, sc.s);
        else if (l.kernel == ATTN_VALU)
            hipk::launchAttentionValu(a, B, sc.s);
        else if (l.kernel == ATTN_MFMA)
            hipk::launchAttentionMfma(a, B, sc.s);
        else
            hipk::launchAttention(a, B, sc.s);
        sc.sync();
        sc.checkGuards();
    };
    if (!l.warmPos.empty()) {  // an earlier launch of other row lengths leaves its partials behind
        const int *measured = a.pos;
        a.pos = sc.upload(l.warmPos);
        run();
        a.pos = measured;
    }
    std::vector<uint8_t> first, firstS;
    for (int r = 0; r < l.repeat; r++) {
        if (r > 0 || !l.warmPos.empty()) {  // same scratch, same output buffer, re-filled with the guard pattern
            DL_HIP(hipMemsetAsync(outBuf, Scratch::kGuardByte, outBytes, sc.s));
            if (a.outS) DL_HIP(hipMemsetAsync(a.outS, Scratch::kGuardByte, sBytes, sc.s));
        }
        run();
        const std::vector<int> cnt = sc.download(a.counters, nCnt);
        for (size_t i = 0; i < nCnt; i++)
            DL_CHECK(cnt[i] == 0, "ops: attention arrival counter " + std::to_string(i) + " is " + std::to_string(cnt[i]) +
                                      " after launch " + std::to_string(r) + " (must reset itself to zero)");
        const std::vector<uint8_t> now = sc.download(static_cast<const uint8_t *>(outBuf), outBytes);
        std::vector<uint8_t> nowS;
        if (a.outS) nowS = sc.download(reinterpret_cast<const uint8_t *>(a.outS), sBytes);
        if (r == 0) {
            first = now;
            firstS = nowS;
        } else {
            DL_CHECK(now == first && nowS == firstS,
                     "ops: attention launch " + std::to_string(r) + " on the same scratch differs bitwise from the first");
        }
    }
    res.out.resize((size_t)B * q0);
    for (int b = 0; b < B; b++)
        for (int i = 0; i < q0; i++) {
            const size_t at = (size_t)b * ldO + i;
            if (l.out == ATTN_OUT_Q80)
                res.out[(size_t)b * q0 + i] = (float)reinterpret_cast<const int8_t *>(first.data())[at];
            else if (l.out == ATTN_OUT_F16)
                res.out[(size_t)b * q0 + i] = f16ToF32(reinterpret_cast<const uint16_t *>(first.data())[at]);
            else
                res.out[(size_t)b * q0 + i] = reinterpret_cast<const float *>(first.data())[at];
        }
    if (l.out == ATTN_OUT_Q80) {
        res.scales.resize((size_t)B * (q0 / 32) * 2);
        for (int b = 0; b < B; b++)
            for (int i = 0; i < q0 / 32 * 2; i++)
                res.scales[(size_t)b * (q0 / 32) * 2 + i] = reinterpret_cast<const float *>(firstS.data())[(size_t)b * ldS * 2 + i];
    }
    return res;
}

namespace {

// ids, partials and (zeroed) counters of an argmax over the device rows `logits`
hipk::ArgmaxArgs argmaxArgs(Scratch &sc, const float *logits, int B, int vocab) {
    hipk::ArgmaxArgs g;
    g.logits = logits;
    g.vocab = vocab;
    g.ids = sc.alloc<int>(B);
    g.partV = sc.alloc<float>((size_t)B * 64);
    g.partI = sc.alloc<int>((size_t)B * 64);
    g.counters = sc.alloc<int>(B);
    return g;
}

// The sampler of the filter and mask benches on the device rows `logits`: temperature 0.8, top-p
// 0.9 and a fixed draw per row.
hipk::SampleArgs benchSampleArgs(Scratch &sc, const float *logits, int B, int vocab) {
    hipk::SampleArgs g;
    g.logits = logits;
    g.vocab = vocab;
    std::vector<float> spec((size_t)B * 4, 0.f);
    for (int b = 0; b < B; b++) {
        spec[(size_t)b * 4] = 0.8f;
        spec[(size_t)b * 4 + 1] = 0.9f;
        spec[(size_t)b * 4 + 2] = (float)((b * 37 + 11) % 100) * 0.01f;
    }
    g.spec = reinterpret_cast<const float4 *>(sc.upload(spec));
    g.ids = sc.alloc<int>(B);
    g.scratch.carve(sc.alloc<uint8_t>(hipk::SampleScratch::bytes(B)), B);  // (alloc zero-fills)
    return g;
}

// The logits of the filter and mask benches: sums of 4 uniform draws, a bell shape over about [-8, 8].
std::vector<float> bellLogits(int B, int vocab) {
    std::vector<float> logits((size_t)B * vocab);
    uint32_t r = 12345u;
    for (size_t i = 0; i < logits.size(); i++) {
        float v = 0.f;
        for (int j = 0; j < 4; j++) {
            r = r * 1664525u + 1013904223u;
            v += (float)(r >> 8) * (1.f / 16777216.f);
        }
        logits[i] = (v - 2.f) * 4.f;
    }
    return logits;
}

constexpr int kBenchWarmups = 5;  // untimed launches before each timeEagerUs window of the row benches
constexpr size_t kRowTailGuard = 256;  // guard elements behind the last row of a row op's logits

}  // namespace

std::vector<int> argmax(const std::vector<float> &logits, int B, int vocab) {
    DL_CHECK(B >= 1 && vocab >= 1 && logits.size() == (size_t)B * vocab, "argmax sizes");
    Scratch sc;
    const hipk::ArgmaxArgs g = argmaxArgs(sc, sc.upload(logits), B, vocab);
    hipk::launchArgmax(g, B, sc.s);
    sc.sync();
    return sc.download(g.ids, B);
}

std::vector<int> sample(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &specs) {
    DL_CHECK(B >= 1 && vocab >= 2 && logits.size() == (size_t)B * vocab && specs.size() == (size_t)B * 4,
             "sample sizes");
    Scratch sc;
    hipk::SampleArgs g;
    g.logits = sc.upload(logits);
    g.vocab = vocab;
    g.spec = reinterpret_cast<const float4 *>(sc.upload(specs));
    g.ids = sc.alloc<int>(B);
    void *ss = sc.alloc<uint8_t>(hipk::SampleScratch::bytes(B));
    DL_HIP(hipMemsetAsync(ss, 0, hipk::SampleScratch::bytes(B), sc.s));
    g.scratch.carve(ss, B);
    hipk::launchSample(g, B, sc.s);
    sc.sync();
    return sc.download(g.ids, B);
}

namespace {
hipk::LogprobArgs logprobArgs(Scratch &sc, int B, int vocab, const std::vector<int> &requests) {
    std::vector<float> spec((size_t)B * 4, 0.f);
    for (int b = 0; b < B; b++) spec[(size_t)b * 4 + 3] = (float)requests[b];
    hipk::LogprobArgs g;
    g.vocab = vocab;
    g.spec = reinterpret_cast<const float4 *>(sc.upload(spec));
    g.scratch.carve(sc.alloc<uint8_t>(hipk::LogprobScratch::bytes(B)), B);  // (alloc zero-fills)
    std::vector<hipk::LogprobEntry> fill((size_t)B * hipk::kLogprobSlots, hipk::LogprobEntry{0.f, -2});
    g.out = sc.upload(fill);
    return g;
}
}  // namespace

void logprobs(const std::vector<float> &logits, int B, int vocab, const std::vector<int> &ids,
              const std::vector<int> &requests, std::vector<float> &outLogprobs, std::vector<int> &outIds,
              const std::vector<float> *warmLogits, const std::vector<int> *warmIds, const std::vector<int> *targets) {
    DL_CHECK(B >= 1 && vocab >= 1 && logits.size() == (size_t)B * vocab && ids.size() == (size_t)B &&
                 requests.size() == (size_t)B && (!targets || targets->size() == (size_t)B), "logprobs sizes");
    for (int r : requests) DL_CHECK(r >= 0 && r <= hipk::kLogprobSlots, "logprobs request out of range");
    Scratch sc;
    hipk::LogprobArgs g = logprobArgs(sc, B, vocab, requests);
    if (warmLogits) {
        DL_CHECK(warmIds && warmLogits->size() == logits.size() && warmIds->size() == ids.size(), "logprobs warm sizes");
        g.logits = sc.upload(*warmLogits);
        g.ids = sc.upload(*warmIds);
        hipk::launchLogprobs(g, B, sc.s);
    }
    g.logits = sc.upload(logits);
    g.ids = sc.upload(ids);
    if (targets) g.target = sc.upload(*targets);
    hipk::launchLogprobs(g, B, sc.s);
    sc.sync();
    const std::vector<hipk::LogprobEntry> out = sc.download(g.out, (size_t)B * hipk::kLogprobSlots);
    outLogprobs.resize(out.size());
    outIds.resize(out.size());
    for (size_t i = 0; i < out.size(); i++) {
        outLogprobs[i] = out[i].logprob;
        outIds[i] = out[i].id;
    }
}

void benchLogprobs(const std::vector<float> &logits, int B, int vocab, int k, int iters, double &logprobsUs,
                   double &argmaxUs, bool targets) {
    DL_CHECK(B >= 1 && vocab >= 1 && logits.size() == (size_t)B * vocab && k >= 0 && k <= hipk::kLogprobTop && iters >= 1,
             "bench_logprobs arguments");
    Scratch sc;
    hipk::LogprobArgs g = logprobArgs(sc, B, vocab, std::vector<int>(B, 1 + k));
    g.logits = sc.upload(logits);
    const hipk::ArgmaxArgs am = argmaxArgs(sc, g.logits, B, vocab);
    g.ids = am.ids;
    if (targets) {
        std::vector<int> tg(B);
        for (int b = 0; b < B; b++) tg[b] = (int)((long long)b * 7919 % vocab);
        g.target = sc.upload(tg);
    }
    argmaxUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] { hipk::launchArgmax(am, B, sc.s); });
    logprobsUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] { hipk::launchLogprobs(g, B, sc.s); });
    sc.sync();
}

namespace {
// spec / proc rows and the per-slot state of a LogitProcArgs
hipk::LogitProcArgs logitProcArgs(Scratch &sc, int B, int vocab, const std::vector<float> &temps,
                                  const std::vector<int> &slots, const std::vector<int> &active,
                                  const std::vector<float> &presence, const std::vector<float> &frequency,
                                  const std::vector<uint32_t> &counts, int nSlots, const std::vector<int> &biasIds,
                                  const std::vector<float> &biasVals, const std::vector<int> &nBias) {
    DL_CHECK(B >= 1 && vocab >= 1 && nSlots >= 1, "logit_proc sizes");
    DL_CHECK(temps.size() == (size_t)B && slots.size() == (size_t)B && active.size() == (size_t)B &&
                 presence.size() == (size_t)B && frequency.size() == (size_t)B, "logit_proc: one entry per row");
    DL_CHECK(counts.size() == (size_t)nSlots * vocab, "logit_proc: counts is [slots][vocab]");
    DL_CHECK(biasIds.size() == (size_t)nSlots * hipk::kMaxLogitBias && biasVals.size() == biasIds.size() &&
                 nBias.size() == (size_t)nSlots, "logit_proc: bias is [slots][300]");
    for (int v : slots) DL_CHECK(v >= 0 && v < nSlots, "logit_proc: slot out of range");
    std::vector<hipk::LogitBiasEntry> bias(biasIds.size());
    for (int s = 0; s < nSlots; s++) {
        DL_CHECK(nBias[s] >= 0 && nBias[s] <= hipk::kMaxLogitBias, "logit_proc: at most 300 bias entries per slot");
        for (int j = 0; j < hipk::kMaxLogitBias; j++) {
            const size_t i = (size_t)s * hipk::kMaxLogitBias + j;
            DL_CHECK(j >= nBias[s] || (biasIds[i] >= 0 && biasIds[i] < vocab), "logit_proc: bias id out of range");
            bias[i] = hipk::LogitBiasEntry{biasIds[i], biasVals[i]};
        }
    }
    std::vector<float> spec((size_t)B * 4, 0.f), proc((size_t)B * 4, 0.f);
    for (int b = 0; b < B; b++) {
        spec[(size_t)b * 4] = temps[b];
        proc[(size_t)b * 4] = presence[b];
        proc[(size_t)b * 4 + 1] = frequency[b];
        proc[(size_t)b * 4 + 2] = active[b] ? 1.f : 0.f;
    }
    hipk::LogitProcArgs g;
    g.vocab = vocab;
    g.spec = reinterpret_cast<const float4 *>(sc.upload(spec));
    g.proc = reinterpret_cast<const float4 *>(sc.upload(proc));
    g.slots = sc.upload(slots);
    g.counts = sc.upload(counts);
    g.bias = sc.upload(bias);
    g.nBias = sc.upload(nBias);
    return g;
}
}  // namespace

std::vector<float> logitProc(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                             const std::vector<int> &slots, const std::vector<int> &active,
                             const std::vector<float> &presence, const std::vector<float> &frequency,
                             const std::vector<uint32_t> &counts, int nSlots, const std::vector<int> &biasIds,
                             const std::vector<float> &biasVals, const std::vector<int> &nBias, float fill) {
    DL_CHECK(B >= 1 && vocab >= 1 && logits.size() == (size_t)B * vocab, "logit_proc: logits is [B][vocab]");
    Scratch sc;
    hipk::LogitProcArgs g =
        logitProcArgs(sc, B, vocab, temps, slots, active, presence, frequency, counts, nSlots, biasIds, biasVals, nBias);
    g.logits = sc.upload(logits);
    g.out = sc.uploadGuardedTail(std::vector<float>(logits.size(), fill), kRowTailGuard, "the processed logits");
    hipk::launchLogitProc(g, B, sc.s);
    sc.sync();
    sc.checkGuards();
    return sc.download(g.out, logits.size());
}

std::vector<uint32_t> logitProcCount(const std::vector<uint32_t> &counts, int nSlots, int vocab,
                                     const std::vector<int> &ids, const std::vector<int> &slots,
                                     const std::vector<int> &active) {
    const int B = (int)ids.size();
    DL_CHECK(B >= 1 && vocab >= 1 && nSlots >= 1 && counts.size() == (size_t)nSlots * vocab &&
                 slots.size() == (size_t)B && active.size() == (size_t)B, "logit_proc_count sizes");
    std::vector<int> seen;
    for (int b = 0; b < B; b++) {
        DL_CHECK(slots[b] >= 0 && slots[b] < nSlots, "logit_proc_count: slot out of range");
        if (active[b]) seen.push_back(slots[b]);
    }
    std::sort(seen.begin(), seen.end());
    DL_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "logit_proc_count: one active row per slot");
    Scratch sc;
    std::vector<float> proc((size_t)B * 4, 0.f);
    for (int b = 0; b < B; b++) proc[(size_t)b * 4 + 2] = active[b] ? 1.f : 0.f;
    hipk::LogitProcArgs g;
    g.vocab = vocab;
    g.proc = reinterpret_cast<const float4 *>(sc.upload(proc));
    g.slots = sc.upload(slots);
    g.counts = sc.upload(counts);
    g.ids = sc.upload(ids);
    hipk::launchLogitProcCount(g, B, sc.s);
    sc.sync();
    return sc.download(g.counts, counts.size());
}

void benchLogitProc(int B, int vocab, int nBias, int iters, double &procUs, double &countUs) {
    DL_CHECK(B >= 1 && vocab >= 1 && nBias >= 0 && nBias <= hipk::kMaxLogitBias && nBias <= vocab && iters >= 1,
             "bench_logit_proc arguments");
    Scratch sc;
    std::vector<float> logits((size_t)B * vocab);
    for (size_t i = 0; i < logits.size(); i++) logits[i] = (float)((i * 2654435761u) % 4096) * (1.f / 256.f) - 8.f;
    std::vector<uint32_t> counts((size_t)B * vocab);
    for (size_t i = 0; i < counts.size(); i++) counts[i] = i % 3 == 0 ? (uint32_t)(1 + i % 5) : 0u;
    std::vector<int> slots(B), active(B, 1), ids(B), nb(B, nBias);
    std::vector<int> biasIds((size_t)B * hipk::kMaxLogitBias, 0);
    std::vector<float> biasVals(biasIds.size(), 0.f);
    for (int b = 0; b < B; b++) {
        slots[b] = b;
        ids[b] = (int)(((size_t)b * 7919) % vocab);
        for (int j = 0; j < nBias; j++) {  // distinct ids spread over the row
            biasIds[(size_t)b * hipk::kMaxLogitBias + j] = (int)((size_t)j * vocab / nBias);
            biasVals[(size_t)b * hipk::kMaxLogitBias + j] = (float)(j % 9) - 4.f;
        }
    }
    hipk::LogitProcArgs g = logitProcArgs(sc, B, vocab, std::vector<float>(B, 0.8f), slots, active,
                                          std::vector<float>(B, 0.5f), std::vector<float>(B, 1.5f), counts, B, biasIds,
                                          biasVals, nb);
    g.logits = sc.upload(logits);
    g.out = sc.alloc<float>((size_t)B * vocab);
    g.ids = sc.upload(ids);
    procUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] { hipk::launchLogitProc(g, B, sc.s); });
    countUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] { hipk::launchLogitProcCount(g, B, sc.s); });
    sc.sync();
}

void pool(const std::vector<PoolLaunch> &launches, int dim, int nSlots, const std::vector<float> &normW, float eps,
          std::vector<float> &out, std::vector<float> &acc) {
    DL_CHECK(dim >= 4 && dim % 4 == 0 && nSlots >= 1 && normW.size() == (size_t)dim, "pool: dim % 4 == 0, one weight per element");
    DL_CHECK(out.size() == (size_t)nSlots * dim && acc.size() == out.size(), "pool: out / acc are [nSlots][dim]");
    Scratch sc;
    hipk::PoolArgs g;
    g.ld = g.dim = dim;
    g.normW = sc.upload(normW);
    g.eps = eps;
    g.acc = sc.upload(acc);
    g.out = sc.upload(out);
    g.part = sc.alloc<float>((size_t)nSlots * hipk::kPoolMaxGroups);
    g.counters = sc.alloc<int>(nSlots);  // (alloc zero-fills)
    for (const PoolLaunch &l : launches) {
        const int B = (int)l.slots.size();
        DL_CHECK(B >= 1 && l.x.size() == (size_t)B * dim && (l.add.empty() || l.add.size() == l.x.size()) &&
                     l.flags.size() == (size_t)B && l.counts.size() == (size_t)B, "pool: launch sizes");
        std::vector<hipk::PoolRow> rows(B);
        std::vector<int> idx(B, 0);
        for (int b = 0; b < B; b++) {
            DL_CHECK(!(l.flags[b] & hipk::kPoolTake) || (l.slots[b] >= 0 && l.slots[b] < nSlots), "pool: slot out of range");
            rows[b] = hipk::PoolRow{l.slots[b], l.flags[b] & 15, l.counts[b], 0, 0, {0, 0, 0}};
        }
        if (hipk::poolPlan(rows.data(), idx.data(), B) == 0) continue;  // no row takes part: never enqueued
        g.in = sc.upload(l.x);
        g.add = l.add.empty() ? nullptr : sc.upload(l.add);
        g.rows = sc.upload(rows);
        g.idx = sc.upload(idx);
        g.scale = sc.alloc<float>(B);
        hipk::launchPool(g, B, sc.s);
    }
    sc.sync();
    out = sc.download(g.out, out.size());
    acc = sc.download(g.acc, acc.size());
    for (int c : sc.download(g.counters, nSlots)) DL_CHECK(c == 0, "pool: a slot's counter is not back to zero");
}

void benchPool(int B, int dim, int slots, bool withAdd, int iters, double &poolUs, double &copyUs) {
    DL_CHECK(B >= 1 && dim >= 4 && dim % 4 == 0 && slots >= 1 && slots <= B && iters >= 1, "bench_pool arguments");
    Scratch sc;
    std::vector<float> x((size_t)B * dim);
    for (size_t i = 0; i < x.size(); i++) x[i] = (float)((i * 2654435761u >> 8) & 1023) / 512.f - 1.f;
    std::vector<hipk::PoolRow> rows(B);
    std::vector<int> idx(B, 0);
    const int per = (B + slots - 1) / slots;
    for (int b = 0; b < B; b++) {
        const int s = b / per, i = b % per, n = std::min(per, B - s * per);
        rows[b] = hipk::PoolRow{s, hipk::kPoolTake | (i == 0 ? hipk::kPoolFirst : 0) | (i == n - 1 ? hipk::kPoolLast : 0), n, 0, 0,
                                {0, 0, 0}};
    }
    hipk::poolPlan(rows.data(), idx.data(), B);
    hipk::PoolArgs g;
    g.ld = g.dim = dim;
    g.normW = sc.upload(std::vector<float>(dim, 1.f));
    g.eps = 1e-5f;
    g.in = sc.upload(x);
    g.add = withAdd ? sc.upload(x) : nullptr;
    g.rows = sc.upload(rows);
    g.idx = sc.upload(idx);
    g.scale = sc.alloc<float>(B);
    g.acc = sc.alloc<float>((size_t)slots * dim);
    g.out = sc.alloc<float>((size_t)slots * dim);
    g.part = sc.alloc<float>((size_t)slots * hipk::kPoolMaxGroups);
    g.counters = sc.alloc<int>(slots);
    float *dst = sc.alloc<float>((size_t)B * dim * (withAdd ? 2 : 1));
    const size_t bytes = (size_t)B * dim * sizeof(float);
    copyUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] {
        DL_HIP(hipMemcpyAsync(dst, g.in, bytes, hipMemcpyDeviceToDevice, sc.s));
        if (withAdd) DL_HIP(hipMemcpyAsync(dst + (size_t)B * dim, g.add, bytes, hipMemcpyDeviceToDevice, sc.s));
    });
    poolUs = timeEagerUs(sc.s, iters, kBenchWarmups, [&] { hipk::launchPool(g, B, sc.s); });
    sc.sync();
}

namespace {
// spec / filter rows and the scratch of a LogitFilterArgs
hipk::LogitFilterArgs logitFilterArgs(Scratch &sc, int B, int vocab, const std::vector<float> &temps,
                                      const std::vector<int> &topK, const std::vector<float> &delta,
                                      const std::vector<int> &active) {
    DL_CHECK(B >= 1 && vocab >= 1, "logit_filter sizes");
    DL_CHECK(temps.size() == (size_t)B && topK.size() == (size_t)B && delta.size() == (size_t)B &&
                 active.size() == (size_t)B, "logit_filter: one entry per row");
    std::vector<float> spec((size_t)B * 4, 0.f);
    std::vector<hipk::LogitFilterRow> rows(B);
    for (int b = 0; b < B; b++) {
        spec[(size_t)b * 4] = temps[b];
        rows[b] = hipk::LogitFilterRow{topK[b], delta[b], active[b] ? 1 : 0, 0};
    }
    hipk::LogitFilterArgs g;
    g.vocab = vocab;
    g.spec = reinterpret_cast<const float4 *>(sc.upload(spec));
    g.rows = sc.upload(rows);
    g.hist = sc.alloc<uint32_t>(hipk::SampleScratch::histFloats(B));
    g.part = sc.alloc<float>((size_t)B * hipk::kSampleMaxGroups);
    g.state = sc.alloc<uint32_t>((size_t)B * hipk::kLogitFilterStateWords);  // (alloc zero-fills)
    return g;
}
}  // namespace

std::vector<float> logitFilter(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                               const std::vector<int> &topK, const std::vector<float> &delta,
                               const std::vector<int> &active) {
    DL_CHECK(B >= 1 && vocab >= 1 && logits.size() == (size_t)B * vocab, "logit_filter: logits is [B][vocab]");
    Scratch sc;
    hipk::LogitFilterArgs g = logitFilterArgs(sc, B, vocab, temps, topK, delta, active);
    g.logits = sc.uploadGuardedTail(logits, kRowTailGuard, "the filtered logits");
    hipk::launchLogitFilter(g, B, sc.s);
    sc.sync();
    sc.checkGuards();
    const std::vector<uint32_t> state = sc.download(g.state, (size_t)B * hipk::kLogitFilterStateWords);
    for (int b = 0; b < B; b++)
        DL_CHECK(state[(size_t)b * hipk::kLogitFilterStateWords + 3] == 0, "logit_filter: a row's counter is not back to zero");
    return sc.download(g.logits, logits.size());
}

namespace {
// The skeleton of the filter and mask benches: fresh rows of bell logits by a D2D copy, one stage on
// them, the sampler on what the stage left. Every figure is a timeEagerUs window of its own.
struct StageBench {
    Scratch &sc;
    int B, iters;
    const float *src;
    float *rows;  // what the stages and the sampler work on
    size_t bytes;
    hipk::SampleArgs sa;
    StageBench(Scratch &sc_, int B_, int vocab, int iters_) : sc(sc_), B(B_), iters(iters_) {
        const std::vector<float> logits = bellLogits(B, vocab);
        src = sc.upload(logits);
        rows = sc.alloc<float>(logits.size());
        bytes = logits.size() * sizeof(float);
        sa = benchSampleArgs(sc, rows, B, vocab);
    }
    void copy() const { DL_HIP(hipMemcpyAsync(rows, src, bytes, hipMemcpyDeviceToDevice, sc.s)); }
    template <typename Launch>
    double launchUs(Launch launch) const { return timeEagerUs(sc.s, iters, kBenchWarmups, launch); }
    double copyUs() const { return launchUs([&] { copy(); }); }
    template <typename Launch>
    double copyStageUs(Launch stage) const {
        return launchUs([&] {
            copy();
            stage();
        });
    }
    double sampleUs() const { return launchUs([&] { hipk::launchSample(sa, B, sc.s); }); }
};
}  // namespace

void benchLogitFilter(int B, int vocab, int topK, float delta, int iters, double &copyUs, double &copyFilterUs,
                      double &sampleUs) {
    DL_CHECK(B >= 1 && vocab >= 2 && iters >= 1, "bench_logit_filter arguments");
    Scratch sc;
    hipk::LogitFilterArgs g = logitFilterArgs(sc, B, vocab, std::vector<float>(B, 0.8f), std::vector<int>(B, topK),
                                              std::vector<float>(B, delta), std::vector<int>(B, 1));
    const StageBench sb(sc, B, vocab, iters);
    g.logits = sb.rows;
    copyUs = sb.copyUs();
    copyFilterUs = sb.copyStageUs([&] { hipk::launchLogitFilter(g, B, sc.s); });
    sampleUs = sb.sampleUs();  // on the filtered rows
    sc.sync();
}

namespace {
// The token table on the device: per token (offset in words, length | class << 16), and the words.
// (`op` names the entry point in the errors)
hipk::TokenTable uploadTokenTable(Scratch &sc, int vocab, const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                                  const std::vector<uint32_t> &words, const std::string &op) {
    DL_CHECK(vocab >= 1 && off.size() == (size_t)vocab && info.size() == (size_t)vocab && !words.empty(), op + ": the table is [vocab]");
    std::vector<uint32_t> meta((size_t)vocab * 2);
    for (int t = 0; t < vocab; t++) {
        const uint32_t len = info[t] & 0xffffu;
        DL_CHECK((size_t)off[t] + (len + 3) / 4 <= words.size(), op + ": a piece lies outside the table's words");
        meta[(size_t)t * 2] = off[t];
        meta[(size_t)t * 2 + 1] = info[t];
    }
    hipk::TokenTable t;
    t.meta = reinterpret_cast<const uint2 *>(sc.upload(meta));
    t.words = sc.upload(words);
    return t;
}

// The rows' spec (temperature, -, -, -) and proc (-, -, -, row kind) entries on the device.
std::pair<const float4 *, const float4 *> uploadDrawRows(Scratch &sc, const std::vector<float> &temps, const std::vector<int> &kinds,
                                                         const std::string &op) {
    static_assert(hipk::kRowKindJson == 1.f && hipk::kRowKindGrammar == 2.f, "row kinds");
    std::vector<float> spec(temps.size() * 4, 0.f), proc(temps.size() * 4, 0.f);
    for (size_t b = 0; b < temps.size(); b++) {
        DL_CHECK(kinds[b] >= 0 && kinds[b] <= 2, op + ": a row's kind is 0 (none), 1 (json) or 2 (grammar)");
        spec[b * 4] = temps[b];
        proc[b * 4 + 3] = (float)kinds[b];
    }
    return {reinterpret_cast<const float4 *>(sc.upload(spec)), reinterpret_cast<const float4 *>(sc.upload(proc))};
}

// The table, the rows and their slots of a ConstraintArgs. The states follow from the entry point:
// jsonArgs, or installGrammars.
hipk::ConstraintArgs constraintArgs(Scratch &sc, const std::string &op, int vocab, const std::vector<float> &temps,
                                    const std::vector<int> &kinds, const std::vector<int> &slots,
                                    const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                                    const std::vector<uint32_t> &words) {
    DL_CHECK(!temps.empty() && kinds.size() == temps.size() && slots.size() == temps.size(), op + ": one temperature, kind and slot per row");
    hipk::ConstraintArgs g;
    g.vocab = vocab;
    std::tie(g.spec, g.proc) = uploadDrawRows(sc, temps, kinds, op);
    g.slots = sc.upload(slots);
    g.table = uploadTokenTable(sc, vocab, off, info, words, op);
    return g;
}

// The JSON entry points' arguments: kind 1 where `on`, row b's slot is b and its state states[4 b ..].
hipk::ConstraintArgs jsonArgs(Scratch &sc, int vocab, const std::vector<float> &temps, const std::vector<int> &on,
                              const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                              const std::vector<uint32_t> &words, const std::vector<uint32_t> &states) {
    const size_t B = temps.size();
    DL_CHECK(on.size() == B && states.size() == B * 4, "json_mask: one temperature, flag and 4-word state per row");
    std::vector<int> kinds(B), slots(B);
    for (size_t b = 0; b < B; b++) {
        kinds[b] = on[b] ? 1 : 0;
        slots[b] = (int)b;
    }
    hipk::ConstraintArgs g = constraintArgs(sc, "json_mask", vocab, temps, kinds, slots, off, info, words);
    g.jsonStates = reinterpret_cast<uint4 *>(sc.upload(states));
    return g;
}

// The grammar entry points' arguments: a table block and a state per slot (a null grammar leaves its
// block zero-filled, which allows nothing). The grammars outlive the call's stream work.
hipk::ConstraintArgs grammarArgs(Scratch &sc, int vocab, const std::vector<float> &temps, const std::vector<int> &kinds,
                                 const std::vector<int> &slots, const std::vector<uint32_t> &off,
                                 const std::vector<uint32_t> &info, const std::vector<uint32_t> &words,
                                 const std::vector<const GrammarDfa *> &grammars, const std::vector<uint32_t> &states) {
    const size_t S = grammars.size();
    DL_CHECK(S >= 1 && states.size() == S, "grammar_mask: one grammar (or none) and one state per slot");
    uint8_t *blocks = sc.alloc<uint8_t>(S * hipk::kGrammarSlotBytes);  // (ahead of the rows and the table, as ever)
    for (size_t s = 0; s < S; s++) {
        if (!grammars[s]) continue;
        const std::string bad = grammarCheck(*grammars[s]);
        DL_CHECK(bad.empty(), "grammar_mask: malformed tables: " + bad);
        hipk::installGrammarTables(blocks + s * hipk::kGrammarSlotBytes, *grammars[s], sc.s);
    }
    // (once, for all slots: without it the bench's advance figure, which is the cost of enqueueing a
    //  launch, was 2 to 3 times the parent's: profiles/draw_stages.md)
    DL_HIP(hipStreamSynchronize(sc.s));
    hipk::ConstraintArgs g = constraintArgs(sc, "grammar_mask", vocab, temps, kinds, slots, off, info, words);
    for (size_t b = 0; b < slots.size(); b++) {
        DL_CHECK(slots[b] >= 0 && (size_t)slots[b] < S, "grammar_mask: slot out of range");
        DL_CHECK(kinds[b] != 2 || grammars[slots[b]], "grammar_mask: a grammar row's slot holds no grammar");
    }
    g.grammarTables = blocks;
    g.grammarStates = sc.upload(states);
    return g;
}
}  // namespace

std::vector<float> jsonMask(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                            const std::vector<int> &on, const std::vector<uint32_t> &off,
                            const std::vector<uint32_t> &info, const std::vector<uint32_t> &words,
                            const std::vector<uint32_t> &states) {
    DL_CHECK(B >= 1 && vocab >= 1 && temps.size() == (size_t)B && logits.size() == (size_t)B * vocab, "json_mask: logits is [B][vocab]");
    Scratch sc;
    hipk::ConstraintArgs g = jsonArgs(sc, vocab, temps, on, off, info, words, states);
    g.logits = sc.uploadGuardedTail(logits, kRowTailGuard, "the masked logits");
    hipk::launchJsonMask(g, B, sc.s);
    sc.sync();
    sc.checkGuards();
    DL_CHECK(sc.download(reinterpret_cast<const uint32_t *>(g.jsonStates), states.size()) == states, "json_mask: the launch changed a state");
    return sc.download(g.logits, logits.size());
}

std::vector<uint32_t> jsonAdvance(int vocab, const std::vector<float> &temps, const std::vector<int> &on,
                                  const std::vector<int> &ids, const std::vector<uint32_t> &off,
                                  const std::vector<uint32_t> &info, const std::vector<uint32_t> &words,
                                  const std::vector<uint32_t> &states) {
    const int B = (int)temps.size();
    DL_CHECK(ids.size() == (size_t)B, "json_advance: one drawn id per row");
    Scratch sc;
    hipk::ConstraintArgs g = jsonArgs(sc, vocab, temps, on, off, info, words, states);
    g.ids = sc.upload(ids);
    hipk::launchJsonAdvance(g, B, sc.s);
    sc.sync();
    return sc.download(reinterpret_cast<const uint32_t *>(g.jsonStates), states.size());
}

void benchJsonMask(int B, int vocab, const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                   const std::vector<uint32_t> &words, const std::vector<uint32_t> &state, int iters, double &copyUs,
                   double &copyMaskUs, double &advanceUs, double &copyFilterUs, double &sampleUs) {
    DL_CHECK(B >= 1 && vocab >= 2 && iters >= 1 && state.size() == 4, "bench_json_mask arguments");
    Scratch sc;
    std::vector<uint32_t> states;
    for (int b = 0; b < B; b++) states.insert(states.end(), state.begin(), state.end());
    hipk::ConstraintArgs g = jsonArgs(sc, vocab, std::vector<float>(B, 0.8f), std::vector<int>(B, 1), off, info, words, states);
    hipk::LogitFilterArgs f = logitFilterArgs(sc, B, vocab, std::vector<float>(B, 0.8f), std::vector<int>(B, 40),
                                              std::vector<float>(B, -INFINITY), std::vector<int>(B, 1));
    const StageBench sb(sc, B, vocab, iters);
    g.logits = f.logits = sb.rows;
    // the advance steps a scratch copy of the states (so that the mask's stay put) by token 0's bytes
    hipk::ConstraintArgs adv = g;
    adv.jsonStates = reinterpret_cast<uint4 *>(sc.upload(states));
    adv.ids = sc.alloc<int>(B);  // (alloc zero-fills)
    copyUs = sb.copyUs();
    copyFilterUs = sb.copyStageUs([&] { hipk::launchLogitFilter(f, B, sc.s); });
    copyMaskUs = sb.copyStageUs([&] { hipk::launchJsonMask(g, B, sc.s); });
    sampleUs = sb.sampleUs();  // on the masked rows
    advanceUs = sb.launchUs([&] { hipk::launchJsonAdvance(adv, B, sc.s); });
    sc.sync();
}

std::vector<float> grammarMask(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                               const std::vector<int> &kinds, const std::vector<int> &slots,
                               const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                               const std::vector<uint32_t> &words, const std::vector<const GrammarDfa *> &grammars,
                               const std::vector<uint32_t> &states) {
    DL_CHECK(B >= 1 && vocab >= 1 && temps.size() == (size_t)B && logits.size() == (size_t)B * vocab, "grammar_mask: logits is [B][vocab]");
    Scratch sc;
    hipk::ConstraintArgs g = grammarArgs(sc, vocab, temps, kinds, slots, off, info, words, grammars, states);
    g.logits = sc.uploadGuardedTail(logits, kRowTailGuard, "the masked logits");
    hipk::launchGrammarMask(g, B, sc.s);
    sc.sync();
    sc.checkGuards();
    const std::vector<uint32_t> after = sc.download(g.grammarStates, states.size());
    DL_CHECK(after == states, "grammar_mask: the launch changed a state");
    return sc.download(g.logits, logits.size());
}

std::vector<uint32_t> grammarAdvance(int vocab, const std::vector<float> &temps, const std::vector<int> &kinds,
                                     const std::vector<int> &slots, const std::vector<int> &ids,
                                     const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                                     const std::vector<uint32_t> &words, const std::vector<const GrammarDfa *> &grammars,
                                     const std::vector<uint32_t> &states) {
    const int B = (int)temps.size();
    DL_CHECK(ids.size() == (size_t)B, "grammar_advance: one drawn id per row");
    std::vector<int> seen;
    for (int b = 0; b < B; b++)
        if (b < (int)kinds.size() && kinds[b] == 2 && temps[b] >= 0.f) seen.push_back(slots[b]);
    std::sort(seen.begin(), seen.end());
    DL_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "grammar_advance: two drawn rows share a slot");
    Scratch sc;
    hipk::ConstraintArgs g = grammarArgs(sc, vocab, temps, kinds, slots, off, info, words, grammars, states);
    g.ids = sc.upload(ids);
    hipk::launchGrammarAdvance(g, B, sc.s);
    sc.sync();
    return sc.download(g.grammarStates, states.size());
}

void benchGrammarMask(int B, int vocab, const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                      const std::vector<uint32_t> &words, const GrammarDfa &grammar, uint32_t state, int iters,
                      double &copyUs, double &copyMaskUs, double &advanceUs, double &copyJsonUs, double &sampleUs) {
    DL_CHECK(B >= 1 && vocab >= 2 && iters >= 1, "bench_grammar_mask arguments");
    Scratch sc;
    std::vector<int> slots(B);
    for (int b = 0; b < B; b++) slots[b] = b;
    const std::vector<float> temps(B, 0.8f);
    const std::vector<uint32_t> states(B, state);
    hipk::ConstraintArgs g = grammarArgs(sc, vocab, temps, std::vector<int>(B, 2), slots, off, info, words,
                                         std::vector<const GrammarDfa *>(B, &grammar), states);
    // the JSON mask on the same rows, every row at START
    hipk::ConstraintArgs j = jsonArgs(sc, vocab, temps, std::vector<int>(B, 1), off, info, words, std::vector<uint32_t>((size_t)B * 4, 0u));
    const StageBench sb(sc, B, vocab, iters);
    g.logits = j.logits = sb.rows;
    // the advance steps a scratch copy of the states (so that the mask's stay put) by token 0's bytes
    hipk::ConstraintArgs adv = g;
    adv.grammarStates = sc.upload(states);
    adv.ids = sc.alloc<int>(B);  // (alloc zero-fills)
    copyUs = sb.copyUs();
    copyJsonUs = sb.copyStageUs([&] { hipk::launchJsonMask(j, B, sc.s); });
    copyMaskUs = sb.copyStageUs([&] { hipk::launchGrammarMask(g, B, sc.s); });
    sampleUs = sb.sampleUs();  // on the masked rows
    advanceUs = sb.launchUs([&] { hipk::launchGrammarAdvance(adv, B, sc.s); });
    sc.sync();
}

std::vector<float> embedding(const std::vector<float> &table, int vocab, int dim, const std::vector<int> &tokens) {
    const int B = (int)tokens.size();
    DL_CHECK(dim % 4 == 0 && table.size() == (size_t)vocab * dim, "embedding sizes");
    for (int t : tokens) DL_CHECK(t >= 0 && t < vocab, "embedding token out of range");
    Scratch sc;
    const float *tab = sc.upload(table);
    const int *tok = sc.upload(tokens);
    float *x = sc.alloc<float>((size_t)B * dim);
    hipk::launchEmbedding(tab, tok, x, dim, B, sc.s);
    sc.sync();
    return sc.download(x, (size_t)B * dim);
}

}  // namespace ops
}  // namespace dl
