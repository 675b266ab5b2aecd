// Python bindings (pybind11) for tests, the torch oracle comparison and bench.py.
// The hot path never goes through Python: a forward call is one C++ call that replays a hipGraph.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "../core/model_file.h"
#include "../core/plan.h"
#include "../core/quant.h"
#include "../core/schema_dfa.h"
#include "../cpu/cpu_ops.h"
#include "../hip/engine.h"
#include "../hip/host_harness.h"
#include "../hip/ops.h"
#include "../runtime/backend.h"
#include "../runtime/weight_stream.h"
#include "../text/tokenizer.h"

namespace py = pybind11;
using namespace dl;

namespace {

py::dict headerToDict(const ModelHeader &h) {
    py::dict d;
    d["header_size"] = h.headerSize;
    d["file_size"] = h.fileSize;
    d["version"] = h.version;
    d["dim"] = h.dim;
    d["hidden_dim"] = h.hiddenDim;
    d["n_layers"] = h.nLayers;
    d["n_heads"] = h.nHeads;
    d["n_kv_heads"] = h.nKvHeads;
    d["n_experts"] = h.nExperts;
    d["vocab_size"] = h.vocabSize;
    d["seq_len"] = h.seqLen;
    d["orig_seq_len"] = h.origSeqLen;
    d["hidden_act"] = (int)h.hiddenAct;
    d["rope_theta"] = h.ropeTheta;
    d["rope_type"] = (int)h.ropeType;
    d["rope_scaling_factor"] = h.ropeScalingFactor;
    d["rope_scaling_low_freq_factor"] = h.ropeScalingLowFreqFactor;
    d["rope_scaling_high_freq_factor"] = h.ropeScalingHighFreqFactor;
    d["rope_scaling_orig_max_seq_len"] = h.ropeScalingOrigMaxSeqLen;
    d["norm_epsilon"] = h.normEpsilon;
    d["weight_type"] = (int)h.weightType;
    d["head_size"] = h.headSize();
    d["kv_dim"] = h.kvDim();
    return d;
}

ModelHeader dictToHeader(const py::dict &d) {
    ModelHeader h;
    h.dim = d["dim"].cast<u32>();
    h.hiddenDim = d["hidden_dim"].cast<u32>();
    h.nLayers = d["n_layers"].cast<u32>();
    h.nHeads = d["n_heads"].cast<u32>();
    h.nKvHeads = d["n_kv_heads"].cast<u32>();
    h.vocabSize = d["vocab_size"].cast<u32>();
    h.seqLen = d["seq_len"].cast<u32>();
    h.origSeqLen = h.seqLen;
    if (d.contains("rope_theta")) h.ropeTheta = d["rope_theta"].cast<float>();
    if (d.contains("hidden_act")) h.hiddenAct = (HiddenAct)d["hidden_act"].cast<int>();
    if (d.contains("rope_scaling_factor")) h.ropeScalingFactor = d["rope_scaling_factor"].cast<float>();
    if (d.contains("rope_scaling_low_freq_factor"))
        h.ropeScalingLowFreqFactor = d["rope_scaling_low_freq_factor"].cast<float>();
    if (d.contains("rope_scaling_high_freq_factor"))
        h.ropeScalingHighFreqFactor = d["rope_scaling_high_freq_factor"].cast<float>();
    if (d.contains("rope_scaling_orig_max_seq_len"))
        h.ropeScalingOrigMaxSeqLen = d["rope_scaling_orig_max_seq_len"].cast<u32>();
    if (d.contains("rope_type")) h.ropeType = (RopeType)d["rope_type"].cast<int>();
    h.weightType = d.contains("weight_type") ? (FloatType)d["weight_type"].cast<int>() : FloatType::Q40;
    return h;
}

EngineConfig makeConfig(const std::string &model, const std::string &bufferType, int nThreads, u32 maxSeqLen,
                        u32 maxBatch, u32 nSlots, int gpuIndex, bool useGraphs, bool kvBf16, py::object synthetic,
                        u64 seed) {
    EngineConfig c;
    c.modelPath = model;
    c.bufferType = parseFloatType(bufferType);
    c.nThreads = nThreads;
    c.maxSeqLen = maxSeqLen;
    c.maxBatch = maxBatch;
    c.nSlots = nSlots;
    c.gpuIndex = gpuIndex;
    c.useGraphs = useGraphs;
    c.kvBf16 = kvBf16;
    c.seed = seed;
    if (!synthetic.is_none()) {
        c.synthetic = true;
        c.syntheticHeader = dictToHeader(synthetic.cast<py::dict>());
    }
    return c;
}

template <typename T>
std::vector<int> toInts(const T &arr) {
    std::vector<int> v;
    for (auto x : arr) v.push_back(py::cast<int>(x));
    return v;
}

py::array_t<float> runForward(Backend &b, const std::vector<int> &tokens, const std::vector<int> &positions,
                              const std::vector<int> &slots) {
    const int n = (int)tokens.size();
    DL_CHECK(positions.size() == tokens.size() && slots.size() == tokens.size(), "input lengths");
    py::array_t<float> out({n, (int)b.header().vocabSize});
    {
        py::gil_scoped_release rel;
        b.forward(n, tokens.data(), positions.data(), slots.data(), out.mutable_data());
    }
    return out;
}

std::vector<int> runArgmax(Backend &b, const std::vector<int> &tokens, const std::vector<int> &positions,
                           const std::vector<int> &slots) {
    std::vector<int> out(tokens.size());
    py::gil_scoped_release rel;
    b.forwardArgmax((int)tokens.size(), tokens.data(), positions.data(), slots.data(), out.data());
    return out;
}

// A JsonState from / to Python: 4 uint32 words, the struct's 16 bytes (word 0 = lex | aux << 8 |
// ws << 16 | depth << 24, words 2 and 3 the stack); lex 255 = rejected.
JsonState stateFromWords(const std::vector<uint32_t> &w) {
    DL_CHECK(w.size() == 4, "a JSON state is 4 words");
    JsonState s;
    std::memcpy(&s, w.data(), sizeof(s));
    s.pad = 0;
    return s;
}
std::vector<uint32_t> stateToWords(const JsonState &s) {
    std::vector<uint32_t> w(4);
    std::memcpy(w.data(), &s, sizeof(s));
    return w;
}
struct PyJsonTable {
    std::shared_ptr<JsonTokenTable> t;
};
// A compiled grammar (structured outputs) and the token table its masks walk.
struct PyGrammar {
    std::shared_ptr<const GrammarDfa> g;
    std::shared_ptr<JsonTokenTable> t;  // may be null (from_table without one): no mask_host / advance_host
};
SchemaDfaCache &schemaCache() {
    static SchemaDfaCache cache;
    return cache;
}

// Per-row logit processors (Backend LogitProc) from Python: None (no row has one) or a sequence
// of n entries, each None (the row has none) or a dict with the optional keys "presence",
// "frequency", "fresh", "bias" (a dict token id -> value, read when fresh), "top_k", "min_p" and
// "json" (the row is in JSON mode: set_json_table first) and "grammar" (a Grammar the row follows:
// structured outputs; set_json_table first as well).
std::vector<LogitProc> parseProcs(const py::object &o, size_t n) {
    std::vector<LogitProc> procs;
    if (o.is_none()) return procs;
    const py::sequence seq = o.cast<py::sequence>();
    DL_CHECK(seq.size() == n, "logit_procs: one entry (or None) per row");
    procs.resize(n);
    for (size_t i = 0; i < n; i++) {
        const py::object e = seq[i];
        if (e.is_none()) continue;
        const py::dict d = e.cast<py::dict>();
        LogitProc &p = procs[i];
        p.active = true;
        if (d.contains("presence")) p.presence = d["presence"].cast<float>();
        if (d.contains("frequency")) p.frequency = d["frequency"].cast<float>();
        if (d.contains("fresh")) p.fresh = d["fresh"].cast<bool>();
        if (d.contains("top_k") && !d["top_k"].is_none()) p.topK = d["top_k"].cast<int>();
        if (d.contains("min_p") && !d["min_p"].is_none()) p.minP = d["min_p"].cast<float>();
        if (d.contains("json") && !d["json"].is_none()) p.json = d["json"].cast<bool>();
        if (d.contains("grammar") && !d["grammar"].is_none()) p.grammar = d["grammar"].cast<const PyGrammar &>().g;
        if (d.contains("bias") && !d["bias"].is_none())
            for (auto kv : d["bias"].cast<py::dict>()) p.bias.push_back(LogitBias{kv.first.cast<int>(), kv.second.cast<float>()});
    }
    return procs;
}

// Per-row draws: specs from (temperature, topp, coin) lists.
std::vector<int> runSample(Backend &b, const std::vector<int> &tokens, const std::vector<int> &positions,
                           const std::vector<int> &slots, const std::vector<float> &temps,
                           const std::vector<float> &topps, const std::vector<float> &coins,
                           const py::object &logitProcs = py::none()) {
    const size_t n = tokens.size();
    DL_CHECK(temps.size() == n && topps.size() == n && coins.size() == n, "one (temperature, topp, coin) per row");
    std::vector<SampleSpec> specs(n);
    for (size_t i = 0; i < n; i++) specs[i] = SampleSpec{temps[i], topps[i], coins[i], 0.f};
    std::vector<int> out(n);
    const std::vector<LogitProc> procs = parseProcs(logitProcs, n);
    py::gil_scoped_release rel;
    if (!procs.empty()) b.setLogitProcs((int)n, procs.data());
    b.forwardSample((int)n, tokens.data(), positions.data(), slots.data(), specs.data(), out.data());
    return out;
}

// forward_sample plus per-row log-probabilities: top[i] = -1 (no request) or k in 0..20. Returns
// (ids, float32 [n][21] logprobs, int32 [n][21] token ids); see Backend::lastLogprobs. targets: None
// or one token id per row (Backend::setLogprobTargets: >= 0 scores that token on a row that draws none).
py::tuple runLogprobs(Backend &b, const std::vector<int> &tokens, const std::vector<int> &positions,
                      const std::vector<int> &slots, const std::vector<float> &temps, const std::vector<float> &topps,
                      const std::vector<float> &coins, const std::vector<int> &top,
                      const py::object &logitProcs = py::none(), const py::object &targets = py::none()) {
    const size_t n = tokens.size();
    const std::vector<int> tg = targets.is_none() ? std::vector<int>() : targets.cast<std::vector<int>>();
    DL_CHECK(targets.is_none() || tg.size() == n, "targets: one token id (or -1) per row");
    DL_CHECK(positions.size() == n && slots.size() == n && temps.size() == n && topps.size() == n &&
                 coins.size() == n && top.size() == n, "one (temperature, topp, coin, top_logprobs) per row");
    std::vector<SampleSpec> specs(n);
    for (size_t i = 0; i < n; i++) {
        DL_CHECK(top[i] >= -1 && top[i] <= kMaxTopLogprobs, "top_logprobs: -1 (none) or 0..20");
        specs[i] = SampleSpec{temps[i], topps[i], coins[i], top[i] < 0 ? 0.f : 1.f + (float)top[i]};
    }
    std::vector<int> out(n);
    std::vector<TokenLogprob> lp;
    const std::vector<LogitProc> procs = parseProcs(logitProcs, n);
    {
        py::gil_scoped_release rel;
        if (!procs.empty()) b.setLogitProcs((int)n, procs.data());
        if (!tg.empty()) b.setLogprobTargets((int)n, tg.data());
        b.forwardSample((int)n, tokens.data(), positions.data(), slots.data(), specs.data(), out.data());
        lp = b.lastLogprobs();
    }
    lp.resize(n * kLogprobEntries, TokenLogprob{0.f, -1});  // (no row asked: empty)
    py::array_t<float> v({(py::ssize_t)n, (py::ssize_t)kLogprobEntries});
    py::array_t<int> ids({(py::ssize_t)n, (py::ssize_t)kLogprobEntries});
    for (size_t i = 0; i < lp.size(); i++) {
        v.mutable_data()[i] = lp[i].logprob;
        ids.mutable_data()[i] = lp[i].id;
    }
    return py::make_tuple(out, v, ids);
}

// Per-row pooling (Backend PoolSpec) from Python: a sequence of n entries, each None (the row takes
// no part) or a dict with the keys "first", "last", "count" and "mode" ("mean" | "last").
std::vector<PoolSpec> parsePool(const py::object &o, size_t n) {
    std::vector<PoolSpec> pool;
    if (o.is_none()) return pool;
    const py::sequence seq = o.cast<py::sequence>();
    DL_CHECK(seq.size() == n, "pooling: one entry (or None) per row");
    pool.resize(n);
    for (size_t i = 0; i < n; i++) {
        const py::object e = seq[i];
        if (e.is_none()) continue;
        const py::dict d = e.cast<py::dict>();
        PoolSpec &p = pool[i];
        p.active = true;
        if (d.contains("first")) p.first = d["first"].cast<bool>();
        if (d.contains("last")) p.last = d["last"].cast<bool>();
        if (d.contains("count")) p.count = d["count"].cast<int>();
        if (d.contains("mode")) {
            const std::string m = d["mode"].cast<std::string>();
            DL_CHECK(m == "mean" || m == "last", "pooling mode: mean | last");
            p.mode = m == "last" ? PoolMode::LAST : PoolMode::MEAN;
        }
    }
    return pool;
}

// A forward with pooling (Backend::setPooling): temperatures None = an all-embedding forward
// (forwardEmbed), else forwardSample of these rows (a row with temperature < 0 draws nothing).
// Returns (ids, finalised slots, float32 [len(slots)][dim] vectors); see Backend::lastEmbeddings.
py::tuple runEmbed(Backend &b, const std::vector<int> &tokens, const std::vector<int> &positions,
                   const std::vector<int> &slots, const py::object &pooling, const py::object &temps,
                   const py::object &topps, const py::object &coins) {
    const size_t n = tokens.size();
    DL_CHECK(positions.size() == n && slots.size() == n, "input lengths");
    const std::vector<PoolSpec> pool = parsePool(pooling, n);
    std::vector<int> out(n, -1);
    std::vector<SampleSpec> specs;
    if (!temps.is_none()) {
        const std::vector<float> t = temps.cast<std::vector<float>>();
        const std::vector<float> tp = topps.is_none() ? std::vector<float>(n, 0.f) : topps.cast<std::vector<float>>();
        const std::vector<float> c = coins.is_none() ? std::vector<float>(n, 0.f) : coins.cast<std::vector<float>>();
        DL_CHECK(t.size() == n && tp.size() == n && c.size() == n, "one (temperature, topp, coin) per row");
        specs.resize(n);
        for (size_t i = 0; i < n; i++) specs[i] = SampleSpec{t[i], tp[i], c[i], 0.f};
    }
    PooledSlots done;
    {
        py::gil_scoped_release rel;
        if (!pool.empty()) b.setPooling((int)n, pool.data());
        if (specs.empty())
            b.forwardEmbed((int)n, tokens.data(), positions.data(), slots.data());
        else
            b.forwardSample((int)n, tokens.data(), positions.data(), slots.data(), specs.data(), out.data());
        done = b.lastEmbeddings();
    }
    const size_t dim = b.header().dim;
    py::array_t<float> v({(py::ssize_t)done.slots.size(), (py::ssize_t)dim});
    if (!done.values.empty()) std::memcpy(v.mutable_data(), done.values.data(), done.values.size() * sizeof(float));
    return py::make_tuple(out, done.slots, v);
}

// Device communicator owned from Python (xGMI one-shot collectives); shared with engines.
struct PyComm {
    std::shared_ptr<DeviceComm> comm;
};
struct PyRcclComm : PyComm {};
struct PyComputeOnlyComm : PyComm {};

// Keeps the device comm alive as long as the engine.
struct PyHipEngine {
    std::shared_ptr<DeviceComm> comm;
    std::unique_ptr<HipEngine> engine;
    int launched = 0;  // rows of the launch_ids forward not collected yet
};


template <typename T>
std::vector<T> vec(const py::object &o) {  // None -> empty
    if (o.is_none()) return {};
    py::array_t<T, py::array::c_style | py::array::forcecast> a(o);
    return std::vector<T>(a.data(), a.data() + a.size());
}

template <typename T>
py::array_t<T> arr(const std::vector<T> &v, std::vector<py::ssize_t> shape) {
    py::array_t<T> a(shape);
    DL_CHECK((size_t)a.size() == v.size(), "result shape");
    std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
    return a;
}

// Test helper of the collectives: x goes to the device, run(in, out, stream) gets it next to
// `outFloats` zeros and returns the device vector (in or out) of `outFloats` floats to hand back.
template <typename Run>
py::array_t<float> hostCollective(const py::array_t<float, py::array::c_style | py::array::forcecast> &x, size_t outFloats,
                                  Run run) {
    std::vector<float> h(x.data(), x.data() + x.size());
    {
        py::gil_scoped_release rel;
        Scratch sc;
        float *in = sc.upload(h);
        h = sc.download(run(in, sc.alloc<float>(outFloats), sc.s), outFloats);
    }
    return arr(h, {(py::ssize_t)outFloats});
}

void bindOps(py::module_ &m) {
    // every py::object is converted to a std::vector while the GIL is held; only the device work
    // runs with it released
    py::module_ o = m.def_submodule("ops", "single-kernel entry points (csrc/hip/ops.h) for numerics tests");
    o.def("gemv_q40",
          [](py::object blocks, int rows, int n, py::object x, py::object residual, py::object normW, float eps, int epi,
             int lanes, int passes) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x), res = vec<float>(residual), nw = vec<float>(normW);
              const int B = (int)(in.size() / n);
              std::vector<float> out, xn;
              {
                  py::gil_scoped_release rel;
                  out = ops::gemvQ40(w, rows, n, in, res, nw, eps, B, epi, &xn, lanes, passes);
              }
              py::object xo = py::none();
              if (!xn.empty()) xo = arr(xn, {B, n});
              return py::make_tuple(arr(out, {B, (py::ssize_t)(out.size() / B)}), xo);
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("residual") = py::none(),
          py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f, py::arg("epi") = 0, py::arg("lanes") = 0,
          py::arg("passes") = 0);
    o.def("gemv_q40_q80_in",
          [](py::object blocks, int rows, int n, py::object x, int lanes, int passes) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x);
              const int B = (int)(in.size() / n);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::gemvQ40Q80In(w, rows, n, in, B, lanes, passes);
              }
              return arr(out, {B, rows});
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("lanes") = 0, py::arg("passes") = 0);
    o.def("gemv_q40_swiglu_q80",
          [](py::object blocks, int rows, int n, py::object x, py::object residual, py::object normW, float eps, int lanes,
             int passes) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x), res = vec<float>(residual), nw = vec<float>(normW);
              const int B = (int)(in.size() / n);
              std::vector<int8_t> codes;
              std::vector<float> scales;
              {
                  py::gil_scoped_release rel;
                  ops::gemvQ40SwigluQ80(w, rows, n, in, res, nw, eps, B, lanes, passes, codes, scales);
              }
              return py::make_tuple(arr(codes, {B, (py::ssize_t)rows / 2}), arr(scales, {B, (py::ssize_t)rows / 64, 2}));
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("residual") = py::none(),
          py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f, py::arg("lanes") = 0, py::arg("passes") = 0);
    o.def("gemv_q40_argmax",
          [](py::object blocks, int rows, int n, py::object x, py::object residual, py::object normW, float eps,
             int vocabStart, int lanes, int passes, int repeat) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x), res = vec<float>(residual), nw = vec<float>(normW);
              int id;
              {
                  py::gil_scoped_release rel;
                  id = ops::gemvQ40Argmax(w, rows, n, in, res, nw, eps, vocabStart, lanes, passes, repeat);
              }
              return id;
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("residual") = py::none(),
          py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f, py::arg("vocab_start") = 0, py::arg("lanes") = 0,
          py::arg("passes") = 0, py::arg("repeat") = 1);
    o.def("gemv_f32",
          [](py::object wts, int rows, int n, py::object x, py::object residual, py::object normW, float eps, int pro,
             int epi, int lanes, int passes) {
              const std::vector<float> w = vec<float>(wts), in = vec<float>(x), res = vec<float>(residual),
                                       nw = vec<float>(normW);
              const int B = (int)(in.size() / n);
              std::vector<float> out, xn;
              {
                  py::gil_scoped_release rel;
                  out = ops::gemvF32(w, rows, n, in, res, nw, eps, B, pro, epi, lanes, passes, &xn);
              }
              py::object xo = py::none();
              if (!xn.empty()) xo = arr(xn, {B, n});
              return py::make_tuple(arr(out, {B, (py::ssize_t)(out.size() / B)}), xo);
          },
          py::arg("w"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("residual") = py::none(),
          py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f, py::arg("pro") = 1, py::arg("epi") = 0,
          py::arg("lanes") = 0, py::arg("passes") = 0);
    o.def("gemv_defaults",
          [](int rows, int n, int B, bool q40, int epi) {
              int lanes = 0, passes = 0;
              ops::gemvDefaults(rows, n, B, q40, epi, lanes, passes);
              return py::make_tuple(lanes, passes);
          },
          py::arg("rows"), py::arg("n"), py::arg("batch") = 1, py::arg("q40") = true, py::arg("epi") = 0,
          "(lanes per row, passes) the engine takes for a matrix of this shape; no device needed");
    o.def("tile_q40",
          [](py::object blocks, int rows, int n, int lanes, bool aos) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              std::vector<uint8_t> qs;
              std::vector<uint32_t> d;
              ops::tileQ40Host(w, rows, n, lanes, aos, qs, d);
              return py::make_tuple(arr(qs, {(py::ssize_t)qs.size()}), arr(d, {(py::ssize_t)d.size()}));
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("lanes"), py::arg("aos") = false,
          "the tiled device image (nibble bytes, u32 scale pairs) written by tileQ40 / tileQ40AoS; no device needed");
    o.def("gemm_q40",
          [](py::object blocks, int rows, int n, py::object x, py::object residual, py::object normW, float eps,
             int splits) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x), res = vec<float>(residual), nw = vec<float>(normW);
              const int M = (int)(in.size() / n);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::gemmQ40(w, rows, n, in, res, nw, eps, M, splits);
              }
              return arr(out, {M, rows});
          },
          py::arg("blocks"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("residual") = py::none(),
          py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f, py::arg("splits") = 0);
    o.def("gemm_f32",
          [](py::object wts, int rows, int n, py::object x, py::object normW, float eps) {
              const std::vector<float> w = vec<float>(wts), in = vec<float>(x), nw = vec<float>(normW);
              const int M = (int)(in.size() / n);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::gemmF32(w, rows, n, in, nw, eps, M);
              }
              return arr(out, {M, rows});
          },
          py::arg("w"), py::arg("rows"), py::arg("n"), py::arg("x"), py::arg("norm_w") = py::none(),
          py::arg("eps") = 1e-5f);
    // ops::gemmBatched: `plan_only` returns the launches (and raises the refusals) without a device
    o.def("gemm",
          [](py::object blocks, py::object wf, int rows, int n, int lanes, int input, py::object x, py::object residual,
             py::object normW, float eps, py::object ss, int ssTiles, int ldSS, int epi, py::object resIn,
             py::object resW, int q0, int kv0, int hs, py::object rope, int seqLen, int nSlots, std::vector<int> pos,
             std::vector<int> slot, bool kvBf16, int splits, int fixed, int chunk, bool planOnly) {
              ops::GemmBatchedArgs a;
              a.blocks = vec<uint8_t>(blocks);
              a.wf = vec<float>(wf);
              a.rows = rows;
              a.n = n;
              a.lanes = lanes;
              a.input = input;
              a.in = vec<float>(x);
              a.residual = vec<float>(residual);
              a.normW = vec<float>(normW);
              a.eps = eps;
              a.M = n > 0 ? (int)(a.in.size() / n) : 0;
              a.ss = vec<float>(ss);
              a.ssTiles = ssTiles;
              a.ldSS = ldSS;
              a.epi = epi;
              a.resIn = vec<float>(resIn);
              a.resW = vec<float>(resW);
              a.q0 = q0;
              a.kv0 = kv0;
              a.hs = hs;
              a.rope = vec<float>(rope);
              a.seqLen = seqLen;
              a.nSlots = nSlots;
              a.pos = pos;
              a.slot = slot;
              a.kvBf16 = kvBf16;
              a.splits = splits;
              a.fixed = fixed;
              a.chunk = chunk;
              ops::GemmBatchedResult r;
              {
                  py::gil_scoped_release rel;
                  if (planOnly)
                      r.launches = ops::gemmBatchedPlan(a);
                  else
                      r = ops::gemmBatched(a);
              }
              static const char *const names[] = {"narrow", "l16", "wide", "f32"};
              py::list launches;
              for (const ops::GemmLaunch &l : r.launches) {
                  py::dict d;
                  d["c0"] = l.c0;
                  d["tokens"] = l.M;
                  d["kernel"] = names[l.kernel];
                  d["splits"] = l.splits;
                  d["grid"] = l.grid;
                  launches.append(d);
              }
              py::dict res;
              res["launches"] = launches;
              if (planOnly) return res;
              const py::ssize_t M = a.M;
              res["out"] = arr(r.out, {M, (py::ssize_t)(r.out.size() / M)});
              if (!r.resX.empty()) {
                  res["res_x"] = arr(r.resX, {M, (py::ssize_t)rows});
                  res["ss_out"] = arr(r.ssOut, {(py::ssize_t)(rows + 63) / 64, (py::ssize_t)ldSS});
              }
              if (!r.k.empty()) {
                  res["k"] = arr(r.k, {M, (py::ssize_t)kv0});
                  res["v"] = arr(r.v, {M, (py::ssize_t)kv0});
              }
              return res;
          },
          py::arg("blocks"), py::arg("wf"), py::arg("rows"), py::arg("n"), py::arg("lanes"), py::arg("input"), py::arg("x"),
          py::arg("residual") = py::none(), py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5f,
          py::arg("ss") = py::none(), py::arg("ss_tiles") = 0, py::arg("ld_ss") = 0, py::arg("epi") = 0,
          py::arg("res_in") = py::none(), py::arg("res_w") = py::none(), py::arg("q0") = 0, py::arg("kv0") = 0,
          py::arg("head_size") = 0, py::arg("rope") = py::none(), py::arg("seq_len") = 0, py::arg("n_slots") = 0,
          py::arg("pos") = std::vector<int>(), py::arg("slot") = std::vector<int>(), py::arg("kv_bf16") = true,
          py::arg("splits") = 0, py::arg("fixed") = 0, py::arg("chunk") = 0, py::arg("plan_only") = false);
    o.def("gemm_splits", &ops::gemmSplitsFor, py::arg("rows"), py::arg("n"), py::arg("tokens"), py::arg("lanes") = 0,
          "K splits the GEMM launcher takes for a launch of `tokens`; no device needed");
    o.def("qkv_rope",
          [](py::object blocks, int q0, int kv0, int hs, int n, py::object x, py::object normW, float eps, py::object rope,
             int seqLen, std::vector<int> pos, bool kvBf16, int lanes, int passes) {
              const std::vector<uint8_t> w = vec<uint8_t>(blocks);
              const std::vector<float> in = vec<float>(x), nw = vec<float>(normW), rp = vec<float>(rope);
              std::vector<float> k, v, q;
              {
                  py::gil_scoped_release rel;
                  q = ops::qkvRope(w, q0, kv0, hs, n, in, nw, eps, rp, seqLen, pos, kvBf16, &k, &v, lanes, passes);
              }
              const py::ssize_t B = (py::ssize_t)pos.size();
              return py::make_tuple(arr(q, {B, q0}), arr(k, {B, kv0}), arr(v, {B, kv0}));
          },
          py::arg("blocks"), py::arg("q0"), py::arg("kv0"), py::arg("head_size"), py::arg("n"), py::arg("x"),
          py::arg("norm_w"), py::arg("eps"), py::arg("rope"), py::arg("seq_len"), py::arg("pos"), py::arg("kv_bf16") = true,
          py::arg("lanes") = 0, py::arg("passes") = 0);
    o.def("attention",
          [](py::object q, py::object k, py::object v, int nSlots, int seqLen, int nHeads0, int kvMul, int hs,
             std::vector<int> pos, std::vector<int> slot, bool kvBf16, int impl) {
              const std::vector<float> qv = vec<float>(q), kv = vec<float>(k), vv = vec<float>(v);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::attention(qv, kv, vv, nSlots, seqLen, nHeads0, kvMul, hs, pos, slot, kvBf16, impl);
              }
              return arr(out, {(py::ssize_t)pos.size(), (py::ssize_t)nHeads0 * hs});
          },
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("n_slots"), py::arg("seq_len"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_size"), py::arg("pos"), py::arg("slot"), py::arg("kv_bf16") = true,
          py::arg("impl") = 0);
    // ops::attentionLaunch: `plan_only` returns the plan (and raises the refusals) without a device
    o.def("attention_launch",
          [](py::object q, py::object k, py::object v, int nSlots, int seqLen, int nHeads0, int kvMul, int hs,
             std::vector<int> pos, std::vector<int> slot, bool kvBf16, int kernel, int mode, bool single, int splitGrid,
             int headGroup, int out, int ldq, int ldOut, int pageSize, std::vector<int> pageOf, py::object poisonK,
             py::object poisonV, int repeat, std::vector<int> warmPos, bool planOnly) {
              ops::AttnLaunchArgs a;
              a.warmPos = warmPos;
              a.q = vec<float>(q);
              a.k = vec<float>(k);
              a.v = vec<float>(v);
              a.nSlots = nSlots;
              a.seqLen = seqLen;
              a.nHeads0 = nHeads0;
              a.kvMul = kvMul;
              a.hs = hs;
              a.pos = pos;
              a.slot = slot;
              a.kvBf16 = kvBf16;
              a.kernel = kernel;
              a.mode = mode;
              a.single = single;
              a.splitGrid = splitGrid;
              a.headGroup = headGroup;
              a.out = out;
              a.ldq = ldq;
              a.ldOut = ldOut;
              a.pageSize = pageSize;
              a.pageOf = pageOf;
              a.poisonK = vec<float>(poisonK);
              a.poisonV = vec<float>(poisonV);
              a.repeat = repeat;
              ops::AttnLaunchResult r;
              {
                  py::gil_scoped_release rel;
                  if (planOnly)
                      r.plan = ops::attentionPlan(a);
                  else
                      r = ops::attentionLaunch(a);
              }
              py::dict res;
              res["kernel"] = r.plan.kernel;
              res["hg"] = r.plan.hg;
              res["grid"] = py::make_tuple(r.plan.grid[0], r.plan.grid[1], r.plan.grid[2]);
              res["split_grid"] = r.plan.splitGrid;
              res["chunk_max"] = r.plan.chunkMax;
              res["short_len"] = r.plan.shortLen;
              py::list splits;
              for (size_t b = 0; b < r.plan.nSplit.size(); b++) splits.append(py::make_tuple(r.plan.nSplit[b], r.plan.ch[b]));
              res["splits"] = splits;
              if (planOnly) return res;
              const py::ssize_t B = (py::ssize_t)pos.size(), q0 = (py::ssize_t)nHeads0 * hs;
              res["out"] = arr(r.out, {B, q0});
              if (!r.scales.empty()) res["scales"] = arr(r.scales, {B, q0 / 32, (py::ssize_t)2});
              return res;
          },
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("n_slots"), py::arg("seq_len"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_size"), py::arg("pos"), py::arg("slot"), py::arg("kv_bf16") = true,
          py::arg("kernel") = 0, py::arg("mode") = 0, py::arg("single") = false, py::arg("split_grid") = 0,
          py::arg("head_group") = 0, py::arg("out") = 0, py::arg("ldq") = 0, py::arg("ld_out") = 0,
          py::arg("page_size") = 0, py::arg("page_of") = std::vector<int>(), py::arg("poison_k") = py::none(),
          py::arg("poison_v") = py::none(), py::arg("repeat") = 1, py::arg("warm_pos") = std::vector<int>(),
          py::arg("plan_only") = false);
    o.def("sample",
          [](py::object logits, int B, py::object specs) {
              const std::vector<float> l = vec<float>(logits), sp = vec<float>(specs);
              std::vector<int> ids;
              {
                  py::gil_scoped_release rel;
                  ids = ops::sample(l, B, (int)(l.size() / B), sp);
              }
              return ids;
          });
    o.def("logprobs",
          [](py::object logits, std::vector<int> ids, std::vector<int> requests, py::object warmLogits,
             py::object warmIds, py::object targets) {
              const std::vector<float> l = vec<float>(logits), wl = vec<float>(warmLogits);
              const std::vector<int> wi = vec<int>(warmIds), tg = vec<int>(targets);
              const int B = (int)ids.size();
              DL_CHECK(B >= 1 && l.size() % B == 0, "logprobs: one id per row");
              std::vector<float> v;
              std::vector<int> idx;
              {
                  py::gil_scoped_release rel;
                  ops::logprobs(l, B, (int)(l.size() / B), ids, requests, v, idx, wl.empty() ? nullptr : &wl,
                                wl.empty() ? nullptr : &wi, targets.is_none() ? nullptr : &tg);
              }
              return py::make_tuple(arr(v, {B, (py::ssize_t)kLogprobEntries}), arr(idx, {B, (py::ssize_t)kLogprobEntries}));
          },
          py::arg("logits"), py::arg("ids"), py::arg("requests"), py::arg("warm_logits") = py::none(),
          py::arg("warm_ids") = py::none(), py::arg("targets") = py::none());
    o.def("logit_proc",
          [](py::object logits, std::vector<float> temps, std::vector<int> slots, std::vector<int> active,
             std::vector<float> presence, std::vector<float> frequency, py::object counts, py::object biasIds,
             py::object biasVals, std::vector<int> nBias, float fill) {
              const std::vector<float> l = vec<float>(logits), bv = vec<float>(biasVals);
              const std::vector<uint32_t> c = vec<uint32_t>(counts);
              const std::vector<int> bi = vec<int>(biasIds);
              const int B = (int)temps.size(), S = (int)nBias.size();
              DL_CHECK(B >= 1 && S >= 1 && l.size() % B == 0, "logit_proc: one temperature per row, one count per slot");
              const int vocab = (int)(l.size() / B);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::logitProc(l, B, vocab, temps, slots, active, presence, frequency, c, S, bi, bv, nBias, fill);
              }
              return arr(out, {B, vocab});
          },
          py::arg("logits"), py::arg("temperatures"), py::arg("slots"), py::arg("active"), py::arg("presence"),
          py::arg("frequency"), py::arg("counts"), py::arg("bias_ids"), py::arg("bias_values"), py::arg("n_bias"),
          py::arg("fill"));
    o.def("logit_proc_count",
          [](py::object counts, int nSlots, std::vector<int> ids, std::vector<int> slots, std::vector<int> active) {
              const std::vector<uint32_t> c = vec<uint32_t>(counts);
              DL_CHECK(nSlots >= 1 && c.size() % nSlots == 0, "logit_proc_count: counts is [slots][vocab]");
              const int vocab = (int)(c.size() / nSlots);
              std::vector<uint32_t> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::logitProcCount(c, nSlots, vocab, ids, slots, active);
              }
              return arr(out, {nSlots, vocab});
          },
          py::arg("counts"), py::arg("n_slots"), py::arg("ids"), py::arg("slots"), py::arg("active"));
    o.def("bench_logit_proc",
          [](int B, int vocab, int nBias, int iters) {
              double pu = 0, cu = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchLogitProc(B, vocab, nBias, iters, pu, cu);
              }
              return py::make_tuple(pu, cu);
          },
          py::arg("batch"), py::arg("vocab"), py::arg("n_bias"), py::arg("iters") = 200,
          "(us per launchLogitProc, us per launchLogitProcCount) on batch x vocab logits");
    o.def("logit_filter",
          [](py::object logits, std::vector<float> temps, std::vector<int> topK, std::vector<float> delta,
             std::vector<int> active) {
              const std::vector<float> l = vec<float>(logits);
              const int B = (int)temps.size();
              DL_CHECK(B >= 1 && l.size() % B == 0, "logit_filter: one temperature per row");
              const int vocab = (int)(l.size() / B);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::logitFilter(l, B, vocab, temps, topK, delta, active);
              }
              return arr(out, {B, vocab});
          },
          py::arg("logits"), py::arg("temperatures"), py::arg("top_k"), py::arg("delta"), py::arg("active"));
    o.def("bench_logit_filter",
          [](int B, int vocab, int topK, float delta, int iters) {
              double cu = 0, fu = 0, su = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchLogitFilter(B, vocab, topK, delta, iters, cu, fu, su);
              }
              return py::make_tuple(cu, fu, su);
          },
          py::arg("batch"), py::arg("vocab"), py::arg("top_k"), py::arg("delta"), py::arg("iters") = 200,
          "(us per device copy of the logits, us per copy + launchLogitFilter, us per launchSample on the filtered rows)");
    o.def("json_mask",
          [](py::object logits, std::vector<float> temps, std::vector<int> on, const PyJsonTable &tb,
             std::vector<std::vector<uint32_t>> states) {
              const std::vector<float> l = vec<float>(logits);
              const int B = (int)temps.size();
              DL_CHECK(B >= 1 && l.size() % B == 0 && states.size() == (size_t)B, "json_mask: one temperature and state per row");
              const int vocab = (int)(l.size() / B);
              std::vector<uint32_t> st;
              for (auto &s : states) {
                  const std::vector<uint32_t> w = stateToWords(stateFromWords(s));
                  st.insert(st.end(), w.begin(), w.end());
              }
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::jsonMask(l, B, vocab, temps, on, tb.t->off, tb.t->info, tb.t->words, st);
              }
              return arr(out, {B, vocab});
          },
          py::arg("logits"), py::arg("temperatures"), py::arg("on"), py::arg("table"), py::arg("states"));
    o.def("json_advance",
          [](std::vector<float> temps, std::vector<int> on, std::vector<int> ids, const PyJsonTable &tb,
             std::vector<std::vector<uint32_t>> states) {
              DL_CHECK(states.size() == temps.size(), "json_advance: one state per row");
              std::vector<uint32_t> st;
              for (auto &s : states) {
                  const std::vector<uint32_t> w = stateToWords(stateFromWords(s));
                  st.insert(st.end(), w.begin(), w.end());
              }
              std::vector<uint32_t> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::jsonAdvance(tb.t->vocab(), temps, on, ids, tb.t->off, tb.t->info, tb.t->words, st);
              }
              std::vector<std::vector<uint32_t>> res;
              for (size_t b = 0; b < temps.size(); b++) res.emplace_back(out.begin() + 4 * b, out.begin() + 4 * b + 4);
              return res;
          },
          py::arg("temperatures"), py::arg("on"), py::arg("ids"), py::arg("table"), py::arg("states"));
    o.def("bench_json_mask",
          [](int B, const PyJsonTable &tb, std::vector<uint32_t> state, int iters) {
              double cu = 0, mu = 0, au = 0, fu = 0, su = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchJsonMask(B, tb.t->vocab(), tb.t->off, tb.t->info, tb.t->words, stateToWords(stateFromWords(state)), iters,
                                     cu, mu, au, fu, su);
              }
              return py::make_tuple(cu, mu, au, fu, su);
          },
          py::arg("batch"), py::arg("table"), py::arg("state"), py::arg("iters") = 200,
          "(us per device copy of the logits, per copy + launchJsonMask, per launchJsonAdvance, per copy + "
          "launchLogitFilter with top_k 40, per launchSample on the masked rows), every row in `state`");
    o.def("grammar_mask",
          [](py::object logits, std::vector<float> temps, std::vector<int> kinds, std::vector<int> slots, const PyJsonTable &tb,
             std::vector<py::object> grammars, std::vector<uint32_t> states) {
              const std::vector<float> l = vec<float>(logits);
              const int B = (int)temps.size();
              DL_CHECK(B >= 1 && l.size() % B == 0, "grammar_mask: one temperature per row");
              const int vocab = (int)(l.size() / B);
              std::vector<const GrammarDfa *> gs;
              for (auto &g : grammars) gs.push_back(g.is_none() ? nullptr : g.cast<const PyGrammar &>().g.get());
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::grammarMask(l, B, vocab, temps, kinds, slots, tb.t->off, tb.t->info, tb.t->words, gs, states);
              }
              return arr(out, {B, vocab});
          },
          py::arg("logits"), py::arg("temperatures"), py::arg("kinds"), py::arg("slots"), py::arg("table"), py::arg("grammars"),
          py::arg("states"));
    o.def("grammar_advance",
          [](std::vector<float> temps, std::vector<int> kinds, std::vector<int> slots, std::vector<int> ids, const PyJsonTable &tb,
             std::vector<py::object> grammars, std::vector<uint32_t> states) {
              std::vector<const GrammarDfa *> gs;
              for (auto &g : grammars) gs.push_back(g.is_none() ? nullptr : g.cast<const PyGrammar &>().g.get());
              py::gil_scoped_release rel;
              return ops::grammarAdvance(tb.t->vocab(), temps, kinds, slots, ids, tb.t->off, tb.t->info, tb.t->words, gs, states);
          },
          py::arg("temperatures"), py::arg("kinds"), py::arg("slots"), py::arg("ids"), py::arg("table"), py::arg("grammars"),
          py::arg("states"));
    o.def("bench_grammar_mask",
          [](int B, const PyJsonTable &tb, const PyGrammar &g, uint32_t state, int iters) {
              double cu = 0, mu = 0, au = 0, ju = 0, su = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchGrammarMask(B, tb.t->vocab(), tb.t->off, tb.t->info, tb.t->words, *g.g, state, iters, cu, mu, au, ju, su);
              }
              return py::make_tuple(cu, mu, au, ju, su);
          },
          py::arg("batch"), py::arg("table"), py::arg("grammar"), py::arg("state"), py::arg("iters") = 200,
          "(us per device copy of the logits, per copy + launchGrammarMask, per launchGrammarAdvance, per copy + "
          "launchJsonMask at START, per launchSample on the masked rows), every row in `state`");
    o.def("pool",
          [](py::list launches, int dim, int nSlots, py::array_t<float, py::array::c_style | py::array::forcecast> normW,
             float eps, py::array_t<float, py::array::c_style | py::array::forcecast> outInit,
             py::array_t<float, py::array::c_style | py::array::forcecast> accInit) {
              std::vector<ops::PoolLaunch> ls;
              for (auto item : launches) {
                  const py::dict d = item.cast<py::dict>();
                  ops::PoolLaunch l;
                  auto x = d["x"].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                  l.x.assign(x.data(), x.data() + x.size());
                  if (d.contains("add") && !d["add"].is_none()) {
                      auto a = d["add"].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                      l.add.assign(a.data(), a.data() + a.size());
                  }
                  l.slots = d["slots"].cast<std::vector<int>>();
                  l.flags = d["flags"].cast<std::vector<int>>();
                  l.counts = d["counts"].cast<std::vector<int>>();
                  ls.push_back(std::move(l));
              }
              std::vector<float> w(normW.data(), normW.data() + normW.size());
              std::vector<float> out(outInit.data(), outInit.data() + outInit.size());
              std::vector<float> acc(accInit.data(), accInit.data() + accInit.size());
              {
                  py::gil_scoped_release rel;
                  ops::pool(ls, dim, nSlots, w, eps, out, acc);
              }
              return py::make_tuple(arr(out, {(py::ssize_t)nSlots, (py::ssize_t)dim}), arr(acc, {(py::ssize_t)nSlots, (py::ssize_t)dim}));
          },
          py::arg("launches"), py::arg("dim"), py::arg("n_slots"), py::arg("norm_w"), py::arg("eps"), py::arg("out"),
          py::arg("acc"), "launchPool per entry of launches on one per-slot state: (out, acc) [n_slots][dim]");
    o.def("bench_pool",
          [](int B, int dim, int slots, bool withAdd, int iters) {
              double pu = 0, cu = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchPool(B, dim, slots, withAdd, iters, pu, cu);
              }
              return py::make_tuple(pu, cu);
          },
          py::arg("rows"), py::arg("dim"), py::arg("slots") = 1, py::arg("add") = true, py::arg("iters") = 50,
          "(us per launchPool, us per device copy of the same rows)");
    o.def("bench_logprobs",
          [](py::object logits, int B, int k, int iters, bool targets) {
              const std::vector<float> l = vec<float>(logits);
              double lp = 0, am = 0;
              {
                  py::gil_scoped_release rel;
                  ops::benchLogprobs(l, B, (int)(l.size() / B), k, iters, lp, am, targets);
              }
              return py::make_tuple(lp, am);
          },
          py::arg("logits"), py::arg("batch"), py::arg("k"), py::arg("iters") = 200, py::arg("targets") = false,
          "(us per launchLogprobs, us per launchArgmax) on the same logits");
    o.def("argmax",
          [](py::object logits, int B) {
              const std::vector<float> l = vec<float>(logits);
              std::vector<int> ids;
              {
                  py::gil_scoped_release rel;
                  ids = ops::argmax(l, B, (int)(l.size() / B));
              }
              return ids;
          },
          py::arg("logits"), py::arg("batch"));
    o.def("embedding",
          [](py::object table, int vocab, int dim, std::vector<int> tokens) {
              const std::vector<float> t = vec<float>(table);
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = ops::embedding(t, vocab, dim, tokens);
              }
              return arr(out, {(py::ssize_t)tokens.size(), dim});
          },
          py::arg("table"), py::arg("vocab"), py::arg("dim"), py::arg("tokens"));
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    m.doc() = "MI355X-native distributed Llama engine (native core)";
    bindOps(m);
    m.def("set_log_level", &setLogLevel);
    m.def("hip_device_count", &hipDeviceCount);
    m.def("hip_max_fork_dst", &hipMaxForkDst);

    m.def("f32_to_f16", &f32ToF16);
    m.def("f16_to_f32", &f16ToF32);
    m.def("quantize_q80", [](py::array_t<float, py::array::c_style | py::array::forcecast> x) {
        const u64 n = (u64)x.size();
        py::array_t<uint8_t> out((py::ssize_t)(n / kQBlock * kQ80BlockBytes));
        quantizeQ80(x.data(), reinterpret_cast<BlockQ80 *>(out.mutable_data()), n);
        return out;
    });
    m.def("quantize_q40", [](py::array_t<float, py::array::c_style | py::array::forcecast> x) {
        const u64 n = (u64)x.size();
        py::array_t<uint8_t> out((py::ssize_t)(n / kQBlock * kQ40BlockBytes));
        quantizeQ40(x.data(), reinterpret_cast<BlockQ40 *>(out.mutable_data()), n);
        return out;
    });
    m.def("dequantize_q80", [](py::array_t<uint8_t, py::array::c_style> b) {
        const u64 n = (u64)b.size() / kQ80BlockBytes * kQBlock;
        py::array_t<float> out((py::ssize_t)n);
        dequantizeQ80(reinterpret_cast<const BlockQ80 *>(b.data()), out.mutable_data(), n);
        return out;
    });
    m.def("dequantize_q40", [](py::array_t<uint8_t, py::array::c_style> b) {
        const u64 n = (u64)b.size() / kQ40BlockBytes * kQBlock;
        py::array_t<float> out((py::ssize_t)n);
        dequantizeQ40(reinterpret_cast<const BlockQ40 *>(b.data()), out.mutable_data(), n);
        return out;
    });

    // CPU reference primitives (csrc/cpu/cpu_ops.h) for the reference-golden tests
    py::module_ co = m.def_submodule("cpu_ops", "CPU reference primitives (csrc/cpu/cpu_ops.h)");
    co.def("sample_host", [](py::array_t<float, py::array::c_style | py::array::forcecast> logits, float temp, float topp,
                             float coin) {
        std::vector<float> l(logits.data(), logits.data() + logits.size());
        return sampleHost(l.data(), (int)l.size(), SampleSpec{temp, topp, coin, 0.f});
    });
    co.def("logit_proc_host",
           [](py::array_t<float, py::array::c_style | py::array::forcecast> logits,
              py::array_t<uint32_t, py::array::c_style | py::array::forcecast> counts, float presence, float frequency,
              std::vector<int> biasIds, std::vector<float> biasVals) {
               DL_CHECK(counts.size() == logits.size() && biasIds.size() == biasVals.size(), "logit_proc_host sizes");
               std::vector<LogitBias> bias(biasIds.size());
               for (size_t i = 0; i < bias.size(); i++) bias[i] = LogitBias{biasIds[i], biasVals[i]};
               py::array_t<float> out((py::ssize_t)logits.size());
               logitProcHost(logits.data(), (int)logits.size(), counts.data(), presence, frequency, bias.data(),
                             (int)bias.size(), out.mutable_data());
               return out;
           },
           py::arg("logits"), py::arg("counts"), py::arg("presence"), py::arg("frequency"), py::arg("bias_ids"),
           py::arg("bias_values"));
    co.def("logit_filter_host",
           [](py::array_t<float, py::array::c_style | py::array::forcecast> logits, int topK, float delta) {
               py::array_t<float> out((py::ssize_t)logits.size());
               std::copy(logits.data(), logits.data() + logits.size(), out.mutable_data());
               logitFilterHost(out.mutable_data(), (int)logits.size(), topK, delta);
               return out;
           },
           py::arg("logits"), py::arg("top_k"), py::arg("delta"),
           "One row through logitFilterHost: top_k (0 or >= vocab: off), delta = min_p_delta(T, min_p) (-inf: off).");
    co.def("json_walk",
           [](py::bytes data, py::object state) {
               JsonState s = state.is_none() ? jsonStart() : stateFromWords(state.cast<std::vector<uint32_t>>());
               for (unsigned char c : std::string(data)) s = jsonStep(s, c);
               return stateToWords(s);
           },
           py::arg("data"), py::arg("state") = py::none(),
           "The JSON automaton's state (4 words; word 0 & 255 == 255: rejected) behind `data`, from `state` (None: START).");
    co.def("min_p_delta", &minPDelta, py::arg("temperature"), py::arg("min_p"),
           "T * log(min_p) as float32 (-inf for min_p <= 0): the distance below the row maximum that min_p keeps.");
    co.def("pool_host",
           [](py::array_t<float, py::array::c_style | py::array::forcecast> x, py::array_t<float, py::array::c_style | py::array::forcecast> normW,
              float eps, const std::string &mode, py::object add) {
               DL_CHECK(x.ndim() == 2 && normW.size() == x.shape(1), "pool_host: x is [N][dim], norm_w [dim]");
               DL_CHECK(mode == "mean" || mode == "last", "pooling mode: mean | last");
               const int n = (int)x.shape(0), dim = (int)x.shape(1);
               std::vector<float> a;
               if (!add.is_none()) {
                   auto av = add.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                   DL_CHECK(av.size() == x.size(), "pool_host: add has x's shape");
                   a.assign(av.data(), av.data() + av.size());
               }
               py::array_t<float> out((py::ssize_t)dim);
               poolHost(x.data(), a.empty() ? nullptr : a.data(), n, dim, normW.data(), eps,
                        mode == "last" ? PoolMode::LAST : PoolMode::MEAN, out.mutable_data());
               return out;
           },
           py::arg("x"), py::arg("norm_w"), py::arg("eps"), py::arg("mode") = "mean", py::arg("add") = py::none(),
           "One request's rows through poolHost: the pooled, L2-normalised vector [dim].");
    co.def("logprobs_host", [](py::array_t<float, py::array::c_style | py::array::forcecast> logits, int chosen, int k) {
        std::vector<TokenLogprob> e(kLogprobEntries);
        logprobsHost(logits.data(), (int)logits.size(), chosen, k, e.data());
        py::array_t<float> v((py::ssize_t)kLogprobEntries);
        py::array_t<int> ids((py::ssize_t)kLogprobEntries);
        for (int i = 0; i < kLogprobEntries; i++) {
            v.mutable_data()[i] = e[i].logprob;
            ids.mutable_data()[i] = e[i].id;
        }
        return py::make_tuple(v, ids);
    }, py::arg("logits"), py::arg("chosen"), py::arg("k"));
    co.def("inv_rms", [](py::array_t<float, py::array::c_style | py::array::forcecast> x, float eps) {
        return cpu::invRms(x.data(), (u32)x.size(), eps);
    });
    auto elementwise = [](float (*f)(float)) {
        return [f](py::array_t<float, py::array::c_style | py::array::forcecast> x) {
            py::array_t<float> out(x.size());
            for (py::ssize_t i = 0; i < x.size(); i++) out.mutable_data()[i] = f(x.data()[i]);
            return out;
        };
    };
    co.def("silu", elementwise(&cpu::silu));
    co.def("gelu", elementwise(&cpu::gelu));
    co.def("softmax", [](py::array_t<float, py::array::c_style | py::array::forcecast> x) {
        py::array_t<float> out(x.size());
        std::memcpy(out.mutable_data(), x.data(), x.size() * sizeof(float));
        softmaxInPlace(out.mutable_data(), (u64)x.size());
        return out;
    });
    // the engines' RoPE table ([seqLen][headSize/2] (cos, sin), Llama-3.1 scaling when the header
    // has rope_scaling_factor != 1) for a header dict
    co.def("rope_table", [](py::dict header) {
        const ModelHeader h = dictToHeader(header);
        std::vector<float> t = buildRopeTable(h);
        py::array_t<float> out({(py::ssize_t)h.seqLen, (py::ssize_t)(h.headSize() / 2), (py::ssize_t)2});
        std::memcpy(out.mutable_data(), t.data(), t.size() * sizeof(float));
        return out;
    });
    co.def("rope_apply", [](py::array_t<float, py::array::c_style | py::array::forcecast> x, int pos, int headSize,
                            py::array_t<float, py::array::c_style | py::array::forcecast> table) {
        py::array_t<float> out(x.size());
        std::memcpy(out.mutable_data(), x.data(), x.size() * sizeof(float));
        cpu::ropeApply(out.mutable_data(), (u32)x.size(), (u32)pos, (u32)headSize, table.data());
        return out;
    });
    // y[B][rows] = W . x[b] with W Q40 blocks [rows][cols/32] and x quantized to Q80 (the
    // reference's matmul_Q80_Q40_F32)
    co.def("matmul_q40_q80", [](py::array_t<uint8_t, py::array::c_style> blocks, int rows, int cols,
                                py::array_t<float, py::array::c_style | py::array::forcecast> x, int nThreads) {
        DL_CHECK(cols % kQBlock == 0 && (size_t)blocks.size() == (size_t)rows * cols / kQBlock * kQ40BlockBytes &&
                     x.size() % cols == 0, "matmul_q40_q80 shapes");
        const int B = (int)(x.size() / cols);
        std::vector<BlockQ80> xq((size_t)B * cols / kQBlock);
        quantizeQ80(x.data(), xq.data(), (u64)B * cols);
        std::vector<const BlockQ80 *> xs(B);
        py::array_t<float> out({(py::ssize_t)B, (py::ssize_t)rows});
        std::vector<float *> ys(B);
        for (int b = 0; b < B; b++) {
            xs[b] = xq.data() + (size_t)b * cols / kQBlock;
            ys[b] = out.mutable_data() + (size_t)b * rows;
        }
        ThreadPool pool(nThreads);
        py::gil_scoped_release rel;
        cpu::matmulQ40Q80(reinterpret_cast<const BlockQ40 *>(blocks.data()), rows, cols, xs.data(), B, ys.data(), pool);
        return out;
    }, py::arg("blocks"), py::arg("rows"), py::arg("cols"), py::arg("x"), py::arg("nthreads") = 4);

    m.def("load_header", [](const std::string &path, u32 maxSeqLen) { return headerToDict(loadModelHeader(path, maxSeqLen)); },
          py::arg("path"), py::arg("max_seq_len") = 0);
    m.def("tensor_table", [](const std::string &path) {
        ModelHeader h = loadModelHeader(path);
        py::list l;
        for (const auto &t : buildTensorTable(h)) {
            py::dict d;
            d["name"] = tensorKindName(t.kind);
            d["layer"] = t.layer;
            d["offset"] = t.offset;
            d["bytes"] = t.bytes;
            d["type"] = (int)t.type;
            d["rows"] = t.rows;
            d["cols"] = t.cols;
            l.append(d);
        }
        return l;
    });
    m.def("shard_plan", [](py::dict header, u32 nRanks, u32 rank) {
        ShardPlan p = ShardPlan::make(dictToHeader(header), nRanks, rank);
        py::dict d;
        d["q0"] = p.q0;
        d["kv0"] = p.kv0;
        d["hidden0"] = p.hidden0;
        d["vocab0"] = p.vocab0;
        d["n_heads0"] = p.nHeads0;
        d["n_kv_heads0"] = p.nKvHeads0;
        d["kv_mul"] = p.kvMul;
        return d;
    });
    m.def("rope_table", [](py::dict header) {
        std::vector<float> t = buildRopeTable(dictToHeader(header));
        return py::array_t<float>((py::ssize_t)t.size(), t.data());
    });

    py::class_<Tokenizer>(m, "Tokenizer")
        .def(py::init<const std::string &, bool>(), py::arg("path"), py::arg("verbose") = false)
        .def("encode",
             [](const Tokenizer &t, const std::string &text, bool addBos, bool addSpecial) {
                 return t.encode(text, addBos, addSpecial);
             },
             py::arg("text"), py::arg("add_bos") = true, py::arg("add_special_tokens") = false)
        .def("decode",
             [](Tokenizer &t, int token) -> py::object {
                 std::string out;
                 if (t.decode(token, out)) return py::bytes(out);
                 return py::none();
             })
        .def("reset_decoder", &Tokenizer::resetDecoder)
        .def("is_eos", &Tokenizer::isEos)
        .def("piece", [](const Tokenizer &t, int id) { return py::bytes(t.piece(id)); })
        .def_property_readonly("vocab_size", &Tokenizer::vocabSize)
        .def_property_readonly("bos_id", &Tokenizer::bosId)
        .def_property_readonly("eos_token_ids", &Tokenizer::eosTokenIds)
        .def_property_readonly("chat_template", [](const Tokenizer &t) { return py::bytes(t.chatTemplate()); });

    py::class_<Sampler>(m, "Sampler")
        .def(py::init<int, float, float, u64>())
        .def("sample",
             [](Sampler &s, py::array_t<float, py::array::c_style | py::array::forcecast> logits) {
                 std::vector<float> v(logits.data(), logits.data() + logits.size());
                 return s.sample(v.data());
             })
        .def("set_temp", &Sampler::setTemp)
        .def("set_seed", &Sampler::setSeed);

    py::enum_<EosResult>(m, "EosResult")
        .value("NOT_EOS", EosResult::NOT_EOS)
        .value("MAYBE_EOS", EosResult::MAYBE_EOS)
        .value("EOS", EosResult::EOS);
    py::class_<EosDetector>(m, "EosDetector")
        .def(py::init<std::vector<int>, std::vector<std::string>, int, int>())
        .def("append",
             [](EosDetector &d, int token, py::object piece) {
                 if (piece.is_none()) return d.append(token, nullptr);
                 std::string s = piece.cast<std::string>();
                 return d.append(token, s.c_str());
             })
        .def("get_delta",
             [](EosDetector &d) -> py::object {
                 std::string out;
                 if (d.getDelta(out)) return py::bytes(out);
                 return py::none();
             })
        .def("reset", &EosDetector::reset);

    py::class_<ChatTemplateGenerator>(m, "ChatTemplateGenerator")
        .def(py::init([](const std::string &type, const std::string &tmpl, const std::string &eos) {
                 return new ChatTemplateGenerator(type.empty() ? ChatTemplateType::UNKNOWN : parseChatTemplateType(type),
                                                  tmpl, eos, false);
             }),
             py::arg("type"), py::arg("template"), py::arg("eos"))
        .def_property_readonly("type", [](const ChatTemplateGenerator &g) { return chatTemplateTypeName(g.type()); })
        .def("generate", [](const ChatTemplateGenerator &g, const std::vector<std::pair<std::string, std::string>> &items,
                            bool appendGenerationPrompt) {
            std::vector<ChatItem> its;
            for (auto &p : items) its.push_back(ChatItem{p.first, p.second});
            GeneratedChat c = g.generate(its, appendGenerationPrompt);
            return py::make_tuple(py::bytes(c.content), py::bytes(c.publicPrompt));
        });

    py::class_<PyJsonTable>(m, "JsonTable")
        .def(py::init([](std::vector<py::bytes> pieces, int bosId, std::vector<int> eosIds) {
                 std::vector<std::string> p;
                 for (auto &b : pieces) p.push_back(std::string(b));
                 return PyJsonTable{std::make_shared<JsonTokenTable>(makeJsonTokenTable(p, bosId, eosIds))};
             }),
             py::arg("pieces"), py::arg("bos_id"), py::arg("eos_ids"))
        .def_property_readonly("vocab", [](const PyJsonTable &t) { return t.t->vocab(); })
        .def_property_readonly("bytes", [](const PyJsonTable &t) { return t.t->bytes(); })
        .def("mask_host",
             [](const PyJsonTable &t, py::array_t<float, py::array::c_style | py::array::forcecast> logits,
                std::vector<uint32_t> state) {
                 py::array_t<float> out((py::ssize_t)logits.size());
                 std::copy(logits.data(), logits.data() + logits.size(), out.mutable_data());
                 jsonMaskHost(out.mutable_data(), (int)logits.size(), *t.t, stateFromWords(state));
                 return out;
             },
             py::arg("logits"), py::arg("state"), "One row through jsonMaskHost.")
        .def("advance_host",
             [](const PyJsonTable &t, std::vector<uint32_t> state, int token) {
                 return stateToWords(jsonAdvanceHost(*t.t, stateFromWords(state), token));
             },
             py::arg("state"), py::arg("token"))
        .def("dead_end", [](const PyJsonTable &t) { return jsonDeadEnd(*t.t); });

    py::class_<PyGrammar>(m, "Grammar")
        .def_static("from_schema",
                    [](const std::string &text, py::object table, bool cache) {
                        PyGrammar g;
                        GrammarVocab vocab;
                        if (!table.is_none()) {
                            g.t = table.cast<const PyJsonTable &>().t;
                            vocab = makeGrammarVocab(g.t->off, g.t->info, g.t->words);
                        }
                        json::Value schema;
                        try {
                            schema = json::Value::parse(text);
                        } catch (const std::runtime_error &e) {
                            throw SchemaError(std::string("json_schema: the schema is not JSON: ") + e.what());
                        }
                        const GrammarVocab *vp = g.t ? &vocab : nullptr;
                        g.g = cache ? schemaCache().get(schema, vp) : compileSchemaDfa(schema, vp);
                        return g;
                    },
                    py::arg("text"), py::arg("json_table") = py::none(), py::arg("cache") = false,
                    "Compiles a JSON schema (text). With a JsonTable the dead-end check runs against its vocabulary and "
                    "mask_host / advance_host work; cache=True goes through the process-wide LRU cache of 32 grammars.")
        .def_static("from_table",
                    [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> classOf,
                       py::array_t<uint16_t, py::array::c_style | py::array::forcecast> next, uint32_t start,
                       std::vector<int> accept, py::object table) {
                        DL_CHECK(classOf.size() == 256, "from_table: class_of is 256 bytes");
                        auto d = std::make_shared<GrammarDfa>();
                        std::memcpy(d->classOf, classOf.data(), 256);
                        DL_CHECK(next.ndim() == 2, "from_table: next is [n_states][n_classes]");
                        d->nStates = (uint32_t)next.shape(0);
                        d->nClasses = (uint32_t)next.shape(1);
                        d->next.assign(next.data(), next.data() + next.size());
                        d->start = start;
                        d->accept.assign((d->nStates + 31) / 32, 0);
                        for (int s : accept) {
                            DL_CHECK(s >= 0 && (uint32_t)s < d->nStates, "from_table: an accepting state that is no state");
                            d->accept[s >> 5] |= 1u << (s & 31);
                        }
                        const std::string bad = grammarCheck(*d);
                        if (!bad.empty()) throw Error("from_table: " + bad);
                        PyGrammar g;
                        g.g = d;
                        if (!table.is_none()) g.t = table.cast<const PyJsonTable &>().t;
                        return g;
                    },
                    py::arg("class_of"), py::arg("next"), py::arg("start"), py::arg("accept"), py::arg("json_table") = py::none(),
                    "A grammar from raw tables: class_of uint8[256], next uint16[n_states][n_classes] (0xFFFF: dead), the "
                    "start state and the list of accepting states.")
        .def_property_readonly("n_states", [](const PyGrammar &g) { return g.g->nStates; })
        .def_property_readonly("n_classes", [](const PyGrammar &g) { return g.g->nClasses; })
        .def_property_readonly("start", [](const PyGrammar &g) { return g.g->start; })
        .def("tables",
             [](const PyGrammar &g) {
                 py::array_t<uint8_t> c(256);
                 std::memcpy(c.mutable_data(), g.g->classOf, 256);
                 py::array_t<uint16_t> n({(py::ssize_t)g.g->nStates, (py::ssize_t)g.g->nClasses});
                 std::memcpy(n.mutable_data(), g.g->next.data(), g.g->next.size() * sizeof(uint16_t));
                 std::vector<int> acc;
                 for (uint32_t s = 0; s < g.g->nStates; s++)
                     if (g.g->accepting(s)) acc.push_back((int)s);
                 return py::make_tuple(c, n, g.g->start, acc);
             },
             "(class_of uint8[256], next uint16[n_states][n_classes], start, the accepting states)")
        .def("table_bytes", [](const PyGrammar &g) { return py::bytes(g.g->tableBytes()); })
        .def("same_object", [](const PyGrammar &a, const PyGrammar &b) { return a.g == b.g; }, py::arg("other"))
        .def("walk",
             [](const PyGrammar &g, py::bytes data, py::object state) -> py::object {
                 uint32_t s = state.is_none() ? g.g->start : state.cast<uint32_t>();
                 for (unsigned char c : std::string(data)) {
                     s = g.g->stepByte(s, c);
                     if (s == kGrammarDead) return py::none();
                 }
                 return py::int_(s);
             },
             py::arg("data"), py::arg("state") = py::none(),
             "The state behind `data` from `state` (None: start); None when a byte has no transition.")
        .def("is_accepting", [](const PyGrammar &g, uint32_t s) { return g.g->accepting(s); }, py::arg("state"))
        .def("accepts",
             [](const PyGrammar &g, py::bytes data) {
                 uint32_t s = g.g->start;
                 for (unsigned char c : std::string(data)) {
                     s = g.g->stepByte(s, c);
                     if (s == kGrammarDead) return false;
                 }
                 return g.g->accepting(s);
             },
             py::arg("data"))
        .def("mask_host",
             [](const PyGrammar &g, py::array_t<float, py::array::c_style | py::array::forcecast> logits, uint32_t state) {
                 DL_CHECK(g.t != nullptr, "mask_host: the grammar was made without a JsonTable");
                 py::array_t<float> out((py::ssize_t)logits.size());
                 std::copy(logits.data(), logits.data() + logits.size(), out.mutable_data());
                 grammarMaskHost(out.mutable_data(), (int)logits.size(), *g.t, *g.g, state);
                 return out;
             },
             py::arg("logits"), py::arg("state"), "One row through grammarMaskHost.")
        .def("advance_host",
             [](const PyGrammar &g, uint32_t state, int token) {
                 DL_CHECK(g.t != nullptr, "advance_host: the grammar was made without a JsonTable");
                 return grammarAdvanceHost(*g.t, *g.g, state, token);
             },
             py::arg("state"), py::arg("token"));
    m.def("schema_cache_stats", [] { return py::make_tuple(schemaCache().size(), schemaCache().hits()); },
          "(entries, hits) of the process-wide schema cache that Grammar.from_schema(cache=True) uses");
    py::register_exception<SchemaError>(m, "SchemaError", PyExc_ValueError);

    py::class_<Backend>(m, "Backend")
        .def("set_json_table", [](Backend &b, const PyJsonTable &t) { b.setJsonTable(t.t); }, py::arg("table"))
        .def_property_readonly("header", [](const Backend &b) { return headerToDict(b.header()); })
        .def_property_readonly("name", &Backend::name)
        .def("forward", [](Backend &b, std::vector<int> t, std::vector<int> p, std::vector<int> s) { return runForward(b, t, p, s); },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("forward_sample", &runSample, py::arg("tokens"), py::arg("positions"), py::arg("slots"),
             py::arg("temperatures"), py::arg("topps"), py::arg("coins"), py::arg("logit_procs") = py::none())
        .def("forward_logprobs", &runLogprobs, py::arg("tokens"), py::arg("positions"), py::arg("slots"),
             py::arg("temperatures"), py::arg("topps"), py::arg("coins"), py::arg("top_logprobs"),
             py::arg("logit_procs") = py::none(), py::arg("targets") = py::none())
        .def("forward_argmax", [](Backend &b, std::vector<int> t, std::vector<int> p, std::vector<int> s) { return runArgmax(b, t, p, s); },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("forward_embed", &runEmbed, py::arg("tokens"), py::arg("positions"), py::arg("slots"), py::arg("pooling"),
             py::arg("temperatures") = py::none(), py::arg("topps") = py::none(), py::arg("coins") = py::none())
        // host backends: (final residual rows [n][dim] before the final norm, the final norm's weights [dim])
        .def("forward_hidden",
             [](Backend &b, std::vector<int> t, std::vector<int> p, std::vector<int> s) {
                 DL_CHECK(p.size() == t.size() && s.size() == t.size(), "input lengths");
                 const py::ssize_t n = (py::ssize_t)t.size(), dim = (py::ssize_t)b.header().dim;
                 py::array_t<float> h({n, dim});
                 {
                     py::gil_scoped_release rel;
                     b.forwardHidden((int)n, t.data(), p.data(), s.data(), h.mutable_data(), false, nullptr);
                 }
                 const float *w = b.finalNormWeights();
                 DL_CHECK(w, "backend keeps no host weights");
                 py::array_t<float> nw(dim);
                 std::memcpy(nw.mutable_data(), w, (size_t)dim * sizeof(float));
                 return py::make_tuple(h, nw);
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("last_stats", [](const Backend &b) {
            ForwardStats s = b.lastStats();
            return py::make_tuple(s.computeMs, s.syncMs, s.sentBytes, s.recvBytes, s.xchgMs);
        })
        .def("copy_prefix", &Backend::copyPrefix, py::arg("src"), py::arg("dst"), py::arg("n"))
        .def("fork_prefix",
             [](Backend &b, int src, const std::vector<int> &dsts, int n) { b.forkPrefix(src, dsts.data(), (int)dsts.size(), n); },
             py::arg("src"), py::arg("dsts"), py::arg("n"));

    m.def("cpu_backend",
          [](const std::string &model, const std::string &bufferType, int nThreads, u32 maxSeqLen, u32 maxBatch,
             u32 nSlots) {
              EngineConfig c = makeConfig(model, bufferType, nThreads, maxSeqLen, maxBatch, nSlots, -1, false, false,
                                          py::none(), 1);
              return makeCpuBackend(c, nullptr);
          },
          py::arg("model"), py::arg("buffer_type") = "q80", py::arg("nthreads") = 1, py::arg("max_seq_len") = 0,
          py::arg("max_batch") = 32, py::arg("n_slots") = 1);

    // CPU tensor parallelism in one process (ThreadGroupComm): rank 0's logits of sequential
    // single-token forwards of `tokens` at positions 0.., [n][vocab], and the greedy continuation
    // of `steps` tokens after them (every rank agrees on it).
    m.def("cpu_simulate_tp",
          [](const std::string &model, const std::string &bufferType, int world, std::vector<int> tokens,
             const std::string &syncType, int steps, int nThreads) {
              EngineConfig c = makeConfig(model, bufferType, nThreads, 0, 8, 1, -1, false, false, py::none(), 1);
              c.syncType = parseFloatType(syncType);
              std::vector<float> logits;
              std::vector<int> greedy;
              u32 vocab = 0;
              {
                  py::gil_scoped_release rel;
                  auto comms = ThreadGroupComm::make(world);
                  std::vector<std::unique_ptr<Backend>> bes(world);
                  std::vector<std::string> errs(world);
                  std::vector<std::thread> th;
                  for (int r = 0; r < world; r++)
                      th.emplace_back([&, r] {
                          try {
                              bes[r] = makeCpuBackend(c, comms[r].get());
                              const u32 V = bes[r]->header().vocabSize;
                              std::vector<float> lg(V);
                              int pos = 0, slot0 = 0;
                              for (int t : tokens) {
                                  bes[r]->forward(1, &t, &pos, &slot0, r == 0 ? lg.data() : nullptr);
                                  if (r == 0) {
                                      vocab = V;
                                      logits.insert(logits.end(), lg.begin(), lg.end());
                                  }
                                  pos++;
                              }
                              if (steps > 0) {
                                  // first continuation token from the prompt's last logits (rank 0),
                                  // shared with the other ranks through the comm (exact for ids)
                                  float id = r == 0 ? (float)(std::max_element(lg.begin(), lg.end()) - lg.begin()) : 0.f;
                                  comms[r]->allReduceSum(&id, 1);
                                  int tok = (int)id;
                                  if (r == 0) greedy.push_back(tok);
                                  for (int s = 1; s < steps; s++) {
                                      int next = 0;
                                      bes[r]->forwardArgmax(1, &tok, &pos, &slot0, &next);
                                      pos++;
                                      tok = next;
                                      if (r == 0) greedy.push_back(tok);
                                  }
                              }
                          } catch (const std::exception &e) {
                              errs[r] = e.what();
                          }
                      });
                  for (auto &t : th) t.join();
                  for (auto &e : errs)
                      if (!e.empty()) throw Error("cpu_simulate_tp: " + e);
              }
              py::array_t<float> a({(py::ssize_t)tokens.size(), (py::ssize_t)vocab});
              std::memcpy(a.mutable_data(), logits.data(), logits.size() * 4);
              return py::make_tuple(a, greedy);
          },
          py::arg("model"), py::arg("buffer_type"), py::arg("world"), py::arg("tokens"), py::arg("sync_type") = "f32",
          py::arg("steps") = 0, py::arg("nthreads") = 1);

    m.def("bench_gemv_q40",
          [](int rows, int n, int pro, int epi, int B, int lanes, int passes, int copies, int iters) {
              return benchGemvQ40(rows, n, pro, epi, B, lanes, passes, copies, iters);
          },
          py::arg("rows"), py::arg("n"), py::arg("pro"), py::arg("epi"), py::arg("batch") = 1, py::arg("lanes") = 0,
          py::arg("passes") = 1, py::arg("copies") = 8, py::arg("iters") = 200, py::call_guard<py::gil_scoped_release>());
    m.def("trace_gemv_q40",
          [](int rows, int n, int pro, int epi, int B, int lanes, int passes, int copies, int iters) {
              std::vector<unsigned long long> t;
              double us;
              {
                  py::gil_scoped_release nogil;
                  us = benchGemvQ40(rows, n, pro, epi, B, lanes, passes, copies, iters, &t);
              }
              return py::make_tuple(us, py::array_t<unsigned long long>(t.size(), t.data()));
          },
          py::arg("rows"), py::arg("n"), py::arg("pro"), py::arg("epi"), py::arg("batch") = 1, py::arg("lanes") = 0,
          py::arg("passes") = 0, py::arg("copies") = 8, py::arg("iters") = 20,
          "bench_gemv_q40 with per-workgroup s_memrealtime stamps: (us, u64[iters*grid*8])");
    m.def("bench_gemm_q40", [](int rows, int n, int M, int epi, int copies, int iters) {
              return benchGemmQ40(rows, n, M, epi, copies, iters);
          }, py::arg("rows"), py::arg("n"), py::arg("tokens"), py::arg("epi") = 0,
          py::arg("copies") = 8, py::arg("iters") = 100, py::call_guard<py::gil_scoped_release>());
    m.def("bench_attention",
          [](int nh, int kvm, int hs, int seq, int pos, int B, int copies, int iters, bool kvBf16) {
              return benchAttention(nh, kvm, hs, seq, pos, B, copies, iters, nullptr, kvBf16);
          },
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_size"), py::arg("seq_len"), py::arg("pos"),
          py::arg("batch") = 1, py::arg("copies") = 32, py::arg("iters") = 200, py::arg("kv_bf16") = true,
          py::call_guard<py::gil_scoped_release>());
    m.def("bench_memcpy_d2d", &benchMemcpyD2D, py::arg("bytes"), py::arg("iters") = 20,
          py::call_guard<py::gil_scoped_release>());
    m.def("trace_gemm_q40",
          [](int rows, int n, int M, int epi, int copies, int iters) {
              std::vector<unsigned long long> t;
              double us;
              {
                  py::gil_scoped_release rel;
                  us = benchGemmQ40(rows, n, M, epi, copies, iters, &t);
              }
              return py::make_tuple(us, t, (int)(t.size() / 8 / ((rows + 63) / 64)));
          },
          py::arg("rows"), py::arg("n"), py::arg("tokens"), py::arg("epi") = 0, py::arg("copies") = 8,
          py::arg("iters") = 50,
          "bench_gemm_q40, then one launch with per-workgroup stamps (gemm_dev.h gemmTrace): (us, u64[], splits)");
    m.def("trace_attention",
          [](int nh, int kvm, int hs, int seq, int pos, int B, int copies, int iters) {
              std::vector<unsigned long long> t;
              double us;
              {
                  py::gil_scoped_release rel;
                  us = benchAttention(nh, kvm, hs, seq, pos, B, copies, iters, &t);
              }
              return py::make_tuple(us, t);
          },
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_size"), py::arg("seq_len"), py::arg("pos"),
          py::arg("batch") = 1, py::arg("copies") = 32, py::arg("iters") = 50,
          "bench_attention, then one launch with per-workgroup stamps (kernels.h AttnArgs::trace): (us, u64[])");

    m.def("simulate_tp",
          [](const std::string &model, const std::string &bufferType, int world, std::vector<int> tokens, bool kvBf16,
             int gpuIndex, bool withFlags) -> py::object {
              EngineConfig c = makeConfig(model, bufferType, 1, 0, 8, 1, gpuIndex, false, kvBf16, py::none(), 1);
              std::vector<float> out;
              std::vector<int> blocks;
              {
                  py::gil_scoped_release rel;
                  out = simulateTensorParallel(c, world, tokens, &blocks);
              }
              const size_t vocab = out.size() / tokens.size();
              py::array_t<float> a({(py::ssize_t)tokens.size(), (py::ssize_t)vocab});
              std::memcpy(a.mutable_data(), out.data(), out.size() * 4);
              if (withFlags) return py::make_tuple(a, blocks);
              return a;
          },
          py::arg("model"), py::arg("buffer_type"), py::arg("world"), py::arg("tokens"), py::arg("kv_bf16") = false,
          py::arg("gpu_index") = 0, py::arg("attn_block_flags") = false);

    m.def("simulate_tp_embed",
          [](const std::string &model, const std::string &bufferType, int world, std::vector<int> tokens, int chunk,
             const std::string &mode, bool kvBf16, int gpuIndex) {
              EngineConfig c = makeConfig(model, bufferType, 1, 0, (u32)std::max(8, chunk), 1, gpuIndex, false, kvBf16,
                                          py::none(), 1);
              DL_CHECK(mode == "mean" || mode == "last", "pooling mode: mean | last");
              std::vector<float> out;
              {
                  py::gil_scoped_release rel;
                  out = simulateTensorParallelEmbed(c, world, tokens, chunk, mode == "last" ? PoolMode::LAST : PoolMode::MEAN);
              }
              py::array_t<float> a((py::ssize_t)out.size());
              std::memcpy(a.mutable_data(), out.data(), out.size() * 4);
              return a;
          },
          py::arg("model"), py::arg("buffer_type"), py::arg("world"), py::arg("tokens"), py::arg("chunk") = 1,
          py::arg("mode") = "mean", py::arg("kv_bf16") = false, py::arg("gpu_index") = 0,
          "The embedding of `tokens` on `world` simulated tensor-parallel ranks (the root's vector [dim]).");

    m.def("shard_bytes",
          [](const std::string &model, u32 world, u32 rank) {
              ModelFile f(model);
              const auto ranges = shardByteRanges(f.header(), f.tensors(), ShardPlan::make(f.header(), world, rank));
              u64 t = 0;
              for (auto &r : ranges) t += r.length;
              return t;
          },
          py::arg("model"), py::arg("world"), py::arg("rank"));

    m.def("rccl_unique_id", []() {
        auto v = rcclGetUniqueId();
        return py::bytes(std::string(v.begin(), v.end()));
    });

    py::class_<PyComm>(m, "XgmiComm")
        .def(py::init([](int rank, int world, size_t maxFloats, int gpuIndex) {
                 auto *c = new PyComm();
                 py::gil_scoped_release rel;
                 (void)hipSetDevice(gpuIndex);
                 c->comm = std::shared_ptr<DeviceComm>(makeXgmiComm(rank, world, maxFloats).release());
                 return c;
             }),
             py::arg("rank"), py::arg("world"), py::arg("max_floats"), py::arg("gpu_index") = 0)
        .def("handle", [](PyComm &c) { return py::bytes(xgmiHandle(c.comm.get())); })
        .def("connect",
             [](PyComm &c, const std::vector<py::bytes> &handles) {
                 std::vector<std::string> hs;
                 for (auto &h : handles) hs.push_back(std::string(h));
                 py::gil_scoped_release rel;
                 xgmiConnect(c.comm.get(), hs);
             })
        .def("timed_out", [](PyComm &c) { return xgmiTimedOut(c.comm.get()); })
        .def("set_low_latency", [](PyComm &c, bool on) { xgmiSetLowLatency(c.comm.get(), on); })
        .def("reset_error", [](PyComm &c) { xgmiResetError(c.comm.get()); })
        .def_property_readonly("cross_device", [](PyComm &c) { return xgmiCrossDevice(c.comm.get()); })
        .def_property_readonly("fenced", [](PyComm &c) { return xgmiFenced(c.comm.get()); })
        // µs per in-graph all-reduce of n floats (iters back-to-back collectives in one hipGraph)
        .def("bench_all_reduce",
             [](PyComm &c, size_t n, int iters) {
                 py::gil_scoped_release rel;
                 Scratch sc;
                 float *d = sc.alloc<float>(n);
                 return timeGraphUs(sc.s, iters, [&](int) { c.comm->allReduceSum(d, n, sc.s); });
             },
             py::arg("n"), py::arg("iters") = 200)
        .def_property_readonly("rank", [](PyComm &c) { return c.comm->rank(); })
        .def_property_readonly("world", [](PyComm &c) { return c.comm->size(); })
        // test helpers: host vector in, collective result out (device round trip on a stream of its own)
        .def("all_reduce",
             [](PyComm &c, py::array_t<float, py::array::c_style | py::array::forcecast> x) {
                 const size_t n = (size_t)x.size();
                 return hostCollective(x, n, [&](float *in, float *, hipStream_t s) {
                     c.comm->allReduceSum(in, n, s);
                     return in;
                 });
             })
        .def("all_gather", [](PyComm &c, py::array_t<float, py::array::c_style | py::array::forcecast> x) {
            const size_t n = (size_t)x.size();
            return hostCollective(x, n * c.comm->size(), [&](float *in, float *out, hipStream_t s) {
                c.comm->allGather(in, out, n, s);
                return out;
            });
        })
        // rank 0 gets every rank's x in rank order (other ranks: zeros)
        .def("gather_to_root", [](PyComm &c, py::array_t<float, py::array::c_style | py::array::forcecast> x) {
            const size_t n = (size_t)x.size();
            return hostCollective(x, n * c.comm->size(), [&](float *in, float *out, hipStream_t s) {
                c.comm->gatherToRoot(in, out, n, s);
                return out;
            });
        })
        .def("broadcast_ints", [](PyComm &c, std::vector<int> v, int root) {
            py::gil_scoped_release rel;
            int *d;
            DL_HIP(hipMalloc(&d, v.size() * 4));
            DL_HIP(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
            c.comm->broadcastInts(d, v.size(), root, nullptr);
            DL_HIP(hipMemcpy(v.data(), d, v.size() * 4, hipMemcpyDeviceToHost));
            DL_HIP(hipFree(d));
            return v;
        }, py::arg("values"), py::arg("root") = 0)
        // the engine's separate-collective schedule, eager or captured + replayed (engine.h)
        .def("schedule_check",
             [](PyComm &c, int layers, int rows, int dim, int vocab0, int runs, bool graph) {
                 py::gil_scoped_release rel;
                 return commScheduleCheck(*c.comm, layers, rows, dim, vocab0, runs, graph);
             },
             py::arg("layers") = 4, py::arg("rows") = 4, py::arg("dim") = 4096, py::arg("vocab0") = 1000,
             py::arg("runs") = 3, py::arg("graph") = true);

    // RCCL data plane (the fallback of the xGMI one): same helpers, created from an RCCL unique id
    py::class_<PyRcclComm, PyComm>(m, "RcclComm")
        .def(py::init([](py::bytes uid, int rank, int world, int gpuIndex) {
                 const std::string s = uid;
                 auto *c = new PyRcclComm();
                 py::gil_scoped_release rel;
                 DL_HIP(hipSetDevice(gpuIndex));
                 c->comm = std::shared_ptr<DeviceComm>(
                     makeRcclComm(std::vector<unsigned char>(s.begin(), s.end()), rank, world).release());
                 return c;
             }),
             py::arg("uid"), py::arg("rank") = 0, py::arg("world") = 1, py::arg("gpu_index") = 0);

    // compute-only TP rank (no peers, nothing exchanged): times a TP-N rank's shard on one GPU
    py::class_<PyComputeOnlyComm, PyComm>(m, "ComputeOnlyComm")
        .def(py::init([](int rank, int world, int gpuIndex) {
                 auto *c = new PyComputeOnlyComm();
                 DL_HIP(hipSetDevice(gpuIndex));
                 c->comm = std::shared_ptr<DeviceComm>(makeComputeOnlyComm(rank, world).release());
                 return c;
             }),
             py::arg("rank") = 0, py::arg("world") = 2, py::arg("gpu_index") = 0);

    py::class_<PyHipEngine>(m, "HipEngine")
        .def(py::init([](const std::string &model, const std::string &bufferType, u32 maxSeqLen, u32 maxBatch,
                         u32 nSlots, int gpuIndex, bool useGraphs, bool kvBf16, py::object synthetic, u64 seed,
                         int rank, int world, py::object uid, py::object comm, const std::string &syncType,
                         u32 kvPages, u32 kvPageSize, bool batchInvariant) {
                 EngineConfig c = makeConfig(model, bufferType, 1, maxSeqLen, maxBatch, nSlots, gpuIndex, useGraphs,
                                             kvBf16, synthetic, seed);
                 c.syncType = parseFloatType(syncType);
                 c.kvPages = kvPages;
                 c.kvPageSize = kvPageSize;
                 c.batchInvariant = batchInvariant;
                 auto *e = new PyHipEngine();
                 if (!comm.is_none()) e->comm = comm.cast<PyComm &>().comm;
                 py::gil_scoped_release rel;
                 if (world > 1 && !e->comm) {
                     std::string s;
                     {
                         py::gil_scoped_acquire acq;
                         s = uid.cast<std::string>();
                     }
                     (void)hipSetDevice(gpuIndex >= 0 ? gpuIndex : 0);
                     e->comm = std::shared_ptr<DeviceComm>(
                         makeRcclComm(std::vector<unsigned char>(s.begin(), s.end()), rank, world).release());
                 }
                 e->engine = makeHipEngine(c, e->comm.get());
                 return e;
             }),
             py::arg("model") = "", py::arg("buffer_type") = "q80", py::arg("max_seq_len") = 0,
             py::arg("max_batch") = 32, py::arg("n_slots") = 1, py::arg("gpu_index") = 0, py::arg("use_graphs") = true,
             py::arg("kv_bf16") = true, py::arg("synthetic") = py::none(), py::arg("seed") = 1234, py::arg("rank") = 0,
             py::arg("world") = 1, py::arg("uid") = py::none(), py::arg("comm") = py::none(),
             py::arg("sync_type") = "f32", py::arg("kv_pages") = 0, py::arg("kv_page_size") = 256,
             py::arg("batch_invariant") = false)
        .def_property_readonly("header", [](const PyHipEngine &e) { return headerToDict(e.engine->header()); })
        .def_property_readonly("device_bytes", [](const PyHipEngine &e) { return e.engine->deviceBytes(); })
        .def_property_readonly("tp_fused", [](const PyHipEngine &e) { return e.engine->tpFused(); })
        .def_property_readonly("attn_block", [](const PyHipEngine &e) { return e.engine->attnBlock(); })
        .def_property_readonly("prenorm", [](const PyHipEngine &e) { return e.engine->prenorm(); })
        .def("trace_attn_block",
             [](PyHipEngine &e, int token, int pos, int slot, int layer) {
                 py::gil_scoped_release rel;
                 return e.engine->traceAttnBlock(token, pos, slot, layer);
             },
             py::arg("token"), py::arg("pos"), py::arg("slot") = 0, py::arg("layer") = 1)
        .def_property_readonly("fused_grid_max", [](const PyHipEngine &e) { return e.engine->fusedGridMax(); })
        .def_property_readonly("kv_pages_free", [](const PyHipEngine &e) { return e.engine->kvPagesFree(); })
        .def("tp_batched_fused", [](const PyHipEngine &e, int n) { return e.engine->tpBatchedFused(n); }, py::arg("n"))
        .def_property_readonly("load_stats",
                               [](const PyHipEngine &e) {
                                   const Backend::LoadStats l = e.engine->loadStats();
                                   py::dict d;
                                   d["ms"] = l.ms;
                                   d["file_bytes"] = l.fileBytes;
                                   d["device_bytes"] = l.deviceBytes;
                                   return d;
                               })
        .def("set_json_table", [](PyHipEngine &e, const PyJsonTable &t) { e.engine->setJsonTable(t.t); }, py::arg("table"))
        .def("forward", [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s) { return runForward(*e.engine, t, p, s); },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("forward_sample",
             [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s, std::vector<float> temps,
                std::vector<float> topps, std::vector<float> coins, py::object procs) {
                 return runSample(*e.engine, t, p, s, temps, topps, coins, procs);
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"), py::arg("temperatures"), py::arg("topps"),
             py::arg("coins"), py::arg("logit_procs") = py::none())
        .def("forward_logprobs",
             [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s, std::vector<float> temps,
                std::vector<float> topps, std::vector<float> coins, std::vector<int> top, py::object procs,
                py::object targets) {
                 return runLogprobs(*e.engine, t, p, s, temps, topps, coins, top, procs, targets);
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"), py::arg("temperatures"), py::arg("topps"),
             py::arg("coins"), py::arg("top_logprobs"), py::arg("logit_procs") = py::none(), py::arg("targets") = py::none())
        .def("forward_argmax", [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s) { return runArgmax(*e.engine, t, p, s); },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("forward_embed",
             [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s, py::object pooling,
                py::object temps, py::object topps, py::object coins) {
                 return runEmbed(*e.engine, t, p, s, pooling, temps, topps, coins);
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"), py::arg("pooling"),
             py::arg("temperatures") = py::none(), py::arg("topps") = py::none(), py::arg("coins") = py::none())
        .def("last_stats",
             [](const PyHipEngine &e) {  // (compute ms, sync ms, sent B, recv B, xchg ms) of the last call
                 ForwardStats s = e.engine->lastStats();
                 return py::make_tuple(s.computeMs, s.syncMs, s.sentBytes, s.recvBytes, s.xchgMs);
             })
        .def("decode_greedy",
             [](PyHipEngine &e, int steps, std::vector<int> tokens, std::vector<int> pos, std::vector<int> slots) {
                 const int nSeq = (int)tokens.size();
                 std::vector<int> out((size_t)steps * nSeq);
                 double ms;
                 {
                     py::gil_scoped_release rel;
                     ms = e.engine->decodeGreedyBatch(steps, nSeq, tokens.data(), pos.data(), slots.data(), out.data());
                 }
                 return py::make_tuple(ms, out);
             },
             py::arg("steps"), py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        // prints the per-kernel-class table; with temperatures (and pooling) the sampled forward of
        // these rows instead of the host-logits one; returns {kernel class: device ms}
        .def("profile_forward",
             [](PyHipEngine &e, std::vector<int> t, std::vector<int> p, std::vector<int> s, py::object temps,
                py::object pooling) {
                 if (temps.is_none()) {
                     e.engine->profileForward((int)t.size(), t.data(), p.data(), s.data());
                     return std::map<std::string, double>();
                 }
                 const std::vector<float> tv = temps.cast<std::vector<float>>();
                 DL_CHECK(tv.size() == t.size() && p.size() == t.size() && s.size() == t.size(), "input lengths");
                 std::vector<SampleSpec> specs(t.size());
                 for (size_t i = 0; i < t.size(); i++) specs[i] = SampleSpec{tv[i], 0.f, 0.f, 0.f};
                 const std::vector<PoolSpec> pool = parsePool(pooling, t.size());
                 return e.engine->profileClasses((int)t.size(), t.data(), p.data(), s.data(), specs.data(),
                                                 pool.empty() ? nullptr : pool.data());
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"), py::arg("temperatures") = py::none(),
             py::arg("pooling") = py::none())
        .def("copy_prefix", [](PyHipEngine &e, int src, int dst, int n) { e.engine->copyPrefix(src, dst, n); },
             py::arg("src"), py::arg("dst"), py::arg("n"))
        .def("fork_prefix",
             [](PyHipEngine &e, int src, const std::vector<int> &dsts, int n) {
                 e.engine->forkPrefix(src, dsts.data(), (int)dsts.size(), n);
             },
             py::arg("src"), py::arg("dsts"), py::arg("n"))
        // a greedy forward launched and left in flight until collect_ids (Backend::launchIds / collectIds)
        .def("launch_ids",
             [](PyHipEngine &e, const std::vector<int> &t, const std::vector<int> &p, const std::vector<int> &s) {
                 DL_CHECK(t.size() == p.size() && t.size() == s.size() && !t.empty(), "launch_ids: one position and slot per token");
                 e.engine->launchIds((int)t.size(), t.data(), p.data(), s.data(), nullptr);
                 e.launched = (int)t.size();
             },
             py::arg("tokens"), py::arg("positions"), py::arg("slots"))
        .def("collect_ids", [](PyHipEngine &e) {
            std::vector<int> ids((size_t)e.launched);
            e.engine->collectIds(ids.data());
            e.launched = 0;
            return ids;
        })
        .def("synchronize", [](PyHipEngine &e) { e.engine->synchronize(); });

}
