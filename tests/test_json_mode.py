"""JSON mode (`response_format: json_object`) on the CPU backend: the byte automaton
(`cpu_ops.json_walk`), the token mask `JsonTable.mask_host`, and `dllama-api`.

Ground truth for the automaton is Python's parser, not the code under test: a byte string must end
in DONE iff it decodes as strict UTF-8 and `json.loads` (strict, `parse_constant` raising) returns
a dict, with nesting depth <= 64, whitespace runs (outside strings) <= 8 bytes and nothing behind
the closing brace. The mask's reference is `py_allowed`, written here on top of `py_step`, a Python
automaton that the same document tests pin against `json.loads` first."""
import json
import random
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_logprobs import PROMPTS, _chat, _post
from test_prefix_cache import _start_api

F32 = np.float32
NEG_INF = F32(-np.inf)
MAX_WS, MAX_DEPTH = 8, 64
WS = b" \t\n\r"


# ---------------------------------------------------------------------------- the oracle

def _raise(name):
    raise ValueError(name)


def oracle(data: bytes) -> bool:
    try:
        text = data.decode("utf-8")
        value = json.loads(text, parse_constant=_raise)
    except (ValueError, RecursionError):
        return False
    if not isinstance(value, dict) or not text.endswith("}"):
        return False
    depth = deepest = run = 0
    in_string = escaped = False
    for ch in text:  # (the text parsed: quotes and escapes are well formed)
        if in_string:
            if escaped:
                escaped = False
            elif ch == "\\":
                escaped = True
            elif ch == '"':
                in_string = False
            continue
        run = run + 1 if ch in " \t\n\r" else 0
        if run > MAX_WS:
            return False
        if ch == '"':
            in_string = True
        elif ch in "{[":
            depth += 1
            deepest = max(deepest, depth)
        elif ch in "}]":
            depth -= 1
    return deepest <= MAX_DEPTH


# ---------------------------------------------------------------------------- a Python automaton
# state: (mode tuple, whitespace run, stack tuple of "o" / "a"); None: rejected

PY_START = (("start",), 0, ())


def _py_after(stack, c):
    if not stack:
        return None
    top = stack[-1]
    if c == 0x2C:
        return (("key_next",) if top == "o" else ("value",), 0, stack)
    if c == (0x7D if top == "o" else 0x5D):
        rest = stack[:-1]
        return (("after",) if rest else ("done",), 0, rest)
    return None


def _py_value(stack, c):
    ch = chr(c)
    if ch == '"':
        return (("str", False, None), 0, stack)
    if ch in "{[":
        if len(stack) >= MAX_DEPTH:
            return None
        return (("obj_open",) if ch == "{" else ("arr_open",), 0, stack + ("o" if ch == "{" else "a",))
    if ch == "-":
        return (("num", "minus"), 0, stack)
    if ch == "0":
        return (("num", "zero"), 0, stack)
    if ch in "123456789":
        return (("num", "int"), 0, stack)
    for word in ("true", "false", "null"):
        if ch == word[0]:
            return (("lit", word, 1), 0, stack)
    return None


def py_step(s, c):
    if s is None:
        return None
    mode, ws, stack = s
    k = mode[0]
    if k == "done":
        return None
    if k == "str":
        key, sub = mode[1], mode[2]
        plain = ("str", key, None)
        if sub is None:
            if c == 0x22:
                return (("colon",) if key else ("after",), 0, stack)
            if c == 0x5C:
                return (("str", key, "esc"), 0, stack)
            if 0x20 <= c <= 0x7F:
                return s
            if 0xC2 <= c <= 0xDF:
                return (("str", key, ("u8", 1, 0x80, 0xBF)), 0, stack)
            if 0xE0 <= c <= 0xEF:
                lo, hi = (0xA0, 0xBF) if c == 0xE0 else (0x80, 0x9F) if c == 0xED else (0x80, 0xBF)
                return (("str", key, ("u8", 2, lo, hi)), 0, stack)
            if 0xF0 <= c <= 0xF4:
                lo, hi = (0x90, 0xBF) if c == 0xF0 else (0x80, 0x8F) if c == 0xF4 else (0x80, 0xBF)
                return (("str", key, ("u8", 3, lo, hi)), 0, stack)
            return None
        if sub == "esc":
            if c == 0x75:
                return (("str", key, ("hex", 4)), 0, stack)
            return (plain, 0, stack) if chr(c) in '"\\/bfnrt' else None
        if sub[0] == "hex":
            if chr(c) not in "0123456789abcdefABCDEF":
                return None
            return (("str", key, ("hex", sub[1] - 1)) if sub[1] > 1 else plain, 0, stack)
        _, n, lo, hi = sub
        if not lo <= c <= hi:
            return None
        return (("str", key, ("u8", n - 1, 0x80, 0xBF)) if n > 1 else plain, 0, stack)
    if k == "lit":
        word, at = mode[1], mode[2]
        if c != ord(word[at]):
            return None
        return (("lit", word, at + 1) if at + 1 < len(word) else ("after",), 0, stack)
    if k == "num":
        st, digit = mode[1], 0x30 <= c <= 0x39
        if st == "minus":
            return (("num", "zero" if c == 0x30 else "int"), 0, stack) if digit else None
        if st == "dot":
            return (("num", "frac"), 0, stack) if digit else None
        if st == "e" and c in (0x2B, 0x2D):
            return (("num", "esign"), 0, stack)
        if st in ("e", "esign"):
            return (("num", "exp"), 0, stack) if digit else None
        if digit:
            return None if st == "zero" else s
        if c == 0x2E and st in ("zero", "int"):
            return (("num", "dot"), 0, stack)
        if c in (0x65, 0x45) and st != "exp":
            return (("num", "e"), 0, stack)
        if c in WS:
            return (("after",), 1, stack)
        return _py_after(stack, c)
    if c in WS:
        return None if ws >= MAX_WS else (mode, ws + 1, stack)
    if k == "start":
        return _py_value(stack, c) if c == 0x7B else None
    if k in ("obj_open", "key_next"):
        if k == "obj_open" and c == 0x7D:
            return _py_after(stack, c)
        return (("str", True, None), 0, stack) if c == 0x22 else None
    if k == "colon":
        return (("value",), 0, stack) if c == 0x3A else None
    if k == "arr_open" and c == 0x5D:
        return _py_after(stack, c)
    if k in ("value", "arr_open"):
        return _py_value(stack, c)
    if k == "after":
        return _py_after(stack, c)
    return None


def py_walk(data: bytes, s=PY_START):
    for c in data:
        s = py_step(s, c)
        if s is None:
            return None
    return s


def py_done(s):
    return s is not None and s[0][0] == "done"


def py_allowed(s, token, pieces, bos_id, eos_ids):
    if token in eos_ids:
        return py_done(s)
    return token < bos_id and len(pieces[token]) >= 1 and py_walk(pieces[token], s) is not None


LEX_DONE, LEX_REJECT = 24, 255


def c_lex(words):
    return words[0] & 0xFF


def c_done(C, data: bytes) -> bool:
    return c_lex(C.cpu_ops.json_walk(data)) == LEX_DONE


def c_accepts(C, data: bytes) -> bool:
    return c_lex(C.cpu_ops.json_walk(data)) != LEX_REJECT


# ---------------------------------------------------------------------------- documents

NUMBERS = ["0", "-0", "7", "-12", "1234567890", "0.5", "-0.25", "3.14159", "1e5", "1E5", "1e+5", "2E-7", "-1.5e10",
           "0e0", "0.0E+00", "9.99e-2"]
STRINGS = ["", "a", "key", "hello world", 'quote " backslash \\ slash /', "\b\f\n\r\t", "é", "日本語", "😀 emoji",
           "\u007f", "mix é\n日\\😀", "퟿", "\U0010ffff"]


class Raw(str):
    """A number written out as it stands."""


def random_value(rng, depth):
    r = rng.random()
    if depth <= 0 or r < 0.45:
        pick = rng.randrange(4)
        if pick == 0:
            return Raw(rng.choice(NUMBERS))
        if pick == 1:
            return rng.choice(STRINGS)
        return rng.choice([True, False, None])
    if r < 0.75:
        return {rng.choice(STRINGS): random_value(rng, depth - 1) for _ in range(rng.randrange(4))}
    return [random_value(rng, depth - 1) for _ in range(rng.randrange(4))]


def serialise(v, item_sep, key_sep, indent, ascii_only, level=0):
    if isinstance(v, Raw):
        return str(v)
    if isinstance(v, str):
        return json.dumps(v, ensure_ascii=ascii_only)
    if v is True or v is False or v is None:
        return json.dumps(v)
    nl = "\n" + " " * (indent * (level + 1)) if indent else ""
    end = "\n" + " " * (indent * level) if indent else ""
    if isinstance(v, dict):
        body = [json.dumps(k, ensure_ascii=ascii_only) + key_sep + serialise(x, item_sep, key_sep, indent, ascii_only, level + 1)
                for k, x in v.items()]
        open_, close = "{", "}"
    else:
        body = [serialise(x, item_sep, key_sep, indent, ascii_only, level + 1) for x in v]
        open_, close = "[", "]"
    if not body:
        return open_ + close
    return open_ + nl + (item_sep + nl).join(body) + end + close


def documents(n=120, seed=5):
    rng = random.Random(seed)
    docs = []
    for i in range(n):
        v = {rng.choice(STRINGS): random_value(rng, 4) for _ in range(rng.randrange(5))}
        item_sep, key_sep = rng.choice([(",", ":"), (", ", ": "), (" ,", " : "), (",\t", ":\r\n")])
        indent = rng.choice([0, 0, 1])  # (depth <= 6: a newline and the indent stay within the cap)
        text = serialise(v, item_sep, key_sep, indent, rng.random() < 0.5)
        docs.append(((" " * rng.randrange(3)) + text).encode("utf-8"))
    return docs


def mutations(doc: bytes, rng, n=12):
    out = []
    for _ in range(n):
        b = bytearray(doc)
        at = rng.randrange(len(b))
        kind = rng.randrange(5)
        if kind == 0:
            b[at] = rng.choice(b'{}[]",:\\ \n0123456789-+.eEtfnu/x' + bytes([0x80, 0xBF, 0xC1, 0xE0, 0xED, 0xF4, 0xFF, 0x1F]))
        elif kind == 1:
            del b[at]
        elif kind == 2:
            b.insert(at, rng.choice(b'{}[]",: \t\\0-.e1') if rng.random() < 0.8 else rng.randrange(256))
        elif kind == 3:
            b = b[:at]
        else:
            b[at:at] = b" " * rng.randrange(1, 10)
        out.append(bytes(b))
    return out


def test_documents_and_mutations_against_python_parser(C):
    rng = random.Random(11)
    docs = documents()
    assert all(oracle(d) for d in docs), "the generator writes valid documents"
    seen = {True: 0, False: 0}
    for d in docs:
        for text in [d] + mutations(d, rng):
            want = oracle(text)
            seen[want] += 1
            assert c_done(C, text) == want, text
            assert py_done(py_walk(text)) == want, text
    assert seen[True] > len(docs) and seen[False] > len(docs)  # mutations fall on both sides


def test_every_prefix_of_an_accepted_text_is_accepted(C):
    for d in documents(40, seed=8):
        for cut in range(len(d) + 1):
            assert c_accepts(C, d[:cut]), (d, cut)
            assert py_walk(d[:cut]) is not None
            assert c_done(C, d[:cut]) == (cut == len(d))


def nest(depth):
    """An object whose innermost container sits at `depth`."""
    return b'{"a":' + b"[" * (depth - 1) + b"]" * (depth - 1) + b"}"


CORNERS = [  # (text, ends in DONE, is a prefix)
    (nest(MAX_DEPTH), True, True),
    (nest(MAX_DEPTH + 1), False, False),
    (b'{"a":' + b'{"a":' * (MAX_DEPTH - 1), False, True),
    (b'{"a":' + b'{"a":' * MAX_DEPTH, False, False),
    (b"{" + b" " * MAX_WS + b"}", True, True),
    (b"{" + b" " * (MAX_WS + 1) + b"}", False, False),
    (b" " * MAX_WS + b"{}", True, True),
    (b" " * (MAX_WS + 1) + b"{}", False, False),
    (b'{"a":1' + b"\n" * MAX_WS + b"}", True, True),
    (b'{"a":1' + b"\n" * (MAX_WS + 1), False, False),
    (b'{"a":01}', False, False), (b'{"a":0', False, True), (b'{"a":01', False, False),
    (b'{"a":-}', False, False), (b'{"a":-', False, True),
    (b'{"a":1.}', False, False), (b'{"a":1.', False, True),
    (b'{"a":1e+}', False, False), (b'{"a":1e+', False, True),
    (b'{"a":"\x80"}', False, False), (b'{"a":"\xbf', False, False),
    (b'{"a":"\xe0\x80', False, False), (b'{"a":"\xe0\xa0\x80"}', True, True),
    (b'{"a":"\xed\xa0', False, False), (b'{"a":"\xed\x9f\xbf"}', True, True),
    (b'{"a":"\xf4\x90', False, False), (b'{"a":"\xf4\x8f\xbf\xbf"}', True, True),
    (b'{"a":"\xf0\x8f', False, False), (b'{"a":"\xf0\x90\x80\x80"}', True, True),
    (b'{"a":"\xc1', False, False), (b'{"a":"\xc2\xa9"}', True, True), (b'{"a":"\xf5', False, False),
    (b'{"a":"\\u12G4"}', False, False), (b'{"a":"\\u12g4', False, False), (b'{"a":"\\u12aF"}', True, True),
    (b'{"a":"\\x"}', False, False), (b'{"a":"\x1f"}', False, False), (b'{"a":"\x7f"}', True, True),
    (b"{} ", False, False), (b"{}\n", False, False), (b"{}{", False, False), (b"{}", True, True),
    (b"[]", False, False), (b'"a"', False, False), (b"1", False, False), (b"", False, True),
    (b'{"a":tru}', False, False), (b'{"a":nul', False, True), (b'{"a":NaN}', False, False),
    (b'{"a":1,}', False, False), (b'{,}', False, False), (b'{"a":[1,]}', False, False), (b'{"a" "b"}', False, False),
    (b'{"a":1,"a":2}', True, True), (b'{"a":[1 ,2 ] }', True, True), (b'{"a":[}', False, False),
]


@pytest.mark.parametrize("text,done,prefix", CORNERS)
def test_named_corner_cases(C, text, done, prefix):
    assert c_done(C, text) == done and c_accepts(C, text) == prefix
    assert py_done(py_walk(text)) == done and (py_walk(text) is not None) == prefix
    if done or not prefix:
        assert oracle(text) == done  # (a prefix that is no document is no case for the parser)


# ---------------------------------------------------------------------------- the mask

CORNER_PREFIXES = [b"", b"{", b'{"', b'{"\\', b'{"\\u1', b'{"k":"\xe6\x97', b'{"k":"\xf0', b'{"k":-', b'{"k":0', b'{"k":12',
                   b'{"k":1.', b'{"k":1.5', b'{"k":1e', b'{"k":1e-', b'{"k":1e-2', b'{"k":tr', b'{"k":fals', b'{"k":[',
                   b'{"k":[1', b'{"k":[1,', b'{"k":"v"', b'{"k"', b'{"k":', b"{" + b" " * MAX_WS, b'{"k":1' + b" " * MAX_WS,
                   b'{"a":' + b"[" * (MAX_DEPTH - 1), b'{"a":' + b'{"a":' * (MAX_DEPTH - 1), b"{}", b'{"k":[]}']


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    info = make_tokenizer(str(tmp_path_factory.mktemp("json_tok") / "t.t"), 512)
    return info["tokens"], info["bos_id"], info["eos"]


def mask_prefixes():
    rng = random.Random(3)
    cuts = []
    for d in documents(24, seed=21):
        cuts += [d[:rng.randrange(len(d) + 1)] for _ in range(3)]
    return cuts + CORNER_PREFIXES


def test_json_mask_host_matches_python_allowed(C, synth):
    pieces, bos_id, eos = synth
    assert len(pieces) == 512 and bos_id == 507 and len(eos) == 2
    table = C.JsonTable(pieces, bos_id, eos)
    assert table.vocab == 512 and table.dead_end() == ""
    rng = np.random.default_rng(1)
    for prefix in mask_prefixes():
        x = (np.round(rng.standard_normal(512) * 24) / 4).astype(F32)
        x[rng.integers(0, 512, 6)] = [NEG_INF, F32(-0.0), F32(0.0), F32(np.nan), F32(3e38), F32(1e-42)]
        state, ps = C.cpu_ops.json_walk(prefix), py_walk(prefix)
        assert ps is not None and c_lex(state) != LEX_REJECT
        got = table.mask_host(x, state)
        allowed = np.array([py_allowed(ps, t, pieces, bos_id, eos) for t in range(512)])
        want = np.where(allowed, x, NEG_INF).astype(F32)
        assert got.dtype == F32 and got.tobytes() == want.tobytes(), prefix
        assert allowed.any(), prefix  # no dead end
        for t in range(bos_id, 512):  # specials: only EOS, only in DONE
            assert allowed[t] == (t in eos and py_done(ps))
        if py_done(ps):
            assert allowed.sum() == len(eos)


def test_json_advance_host_follows_the_bytes(C, synth):
    pieces, bos_id, eos = synth
    table = C.JsonTable(pieces, bos_id, eos)
    rng = random.Random(4)
    for prefix in mask_prefixes():
        state, ps = C.cpu_ops.json_walk(prefix), py_walk(prefix)
        for t in [rng.randrange(512) for _ in range(24)] + eos:
            got = table.advance_host(state, t)
            if py_allowed(ps, t, pieces, bos_id, eos):
                assert got == (state if t in eos else C.cpu_ops.json_walk(pieces[t], state)), (prefix, t)
            else:
                assert got == state, (prefix, t)
    assert table.advance_host(C.cpu_ops.json_walk(b"{"), -1) == C.cpu_ops.json_walk(b"{")


def test_dead_end_check_names_a_missing_byte(C, synth):
    pieces, bos_id, eos = synth
    assert "EOS" in C.JsonTable(pieces, bos_id, []).dead_end()
    no_quote = [p if p != b'"' else b"" for p in pieces]
    assert C.JsonTable(no_quote, bos_id, eos).dead_end() != ""
    no_cont = [p if p != b"\x80" else b"" for p in pieces]  # (every continuation range holds other bytes)
    assert C.JsonTable(no_cont, bos_id, eos).dead_end() == ""
    no_digits = [p if not (len(p) == 1 and p.isdigit()) else b"" for p in pieces]
    assert C.JsonTable(no_digits, bos_id, eos).dead_end() != ""


# ---------------------------------------------------------------------------- Backend.forward_sample

def run_json_rows(be, C, table, steps=5):
    """Shared with the GPU test. `steps` decode steps of two requests per slot (the second reuses the
    slots: a fresh row restarts the state): row 0 greedy with penalties, row 1 sampled with a bias and
    top_k 3, row 2 plain. Every constrained draw equals the host pipeline (penalties and bias, mask,
    filter, draw) on `forward`'s own logits for the row, with the state the earlier draws led to."""
    vocab = table.vocab
    for request in range(2):
        states = [C.cpu_ops.json_walk(b""), C.cpu_ops.json_walk(b"")]
        counts = np.zeros(vocab, np.uint32)
        toks = [65 + request, 66]
        for s in range(steps):
            args = (toks + [67], [s, s, s], [0, 1, 2])
            temps, topps, coins = [0.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.0, (0.17 + 0.29 * s) % 1, 0.5]
            raw = be.forward(*args)
            procs = [dict(json=True, fresh=s == 0, presence=0.5, frequency=0.25),
                     dict(json=True, fresh=s == 0, top_k=3, bias={34: 5.0}), None]
            got = be.forward_sample(*args, temps, topps, coins, logit_procs=procs)
            assert got[2] == be.forward_sample(*args, temps, topps, coins)[2]
            row0 = C.cpu_ops.logit_proc_host(raw[0], counts, 0.5, 0.25, [], [])
            row1 = C.cpu_ops.logit_proc_host(raw[1], np.zeros(vocab, np.uint32), 0.0, 0.0, [34], [5.0])
            row1 = C.cpu_ops.logit_filter_host(table.mask_host(row1, states[1]), 3, float("-inf"))
            want = [C.cpu_ops.sample_host(table.mask_host(row0, states[0]), 0.0, 0.9, 0.0),
                    C.cpu_ops.sample_host(row1, temps[1], topps[1], coins[1])]
            assert got[:2] == want, (request, s)
            counts[got[0]] += 1
            for b in range(2):  # (a plain byte inside a string leaves the state as it is)
                assert table.mask_host(np.zeros(vocab, F32), states[b])[got[b]] == 0  # the draw was allowed
                states[b] = table.advance_host(states[b], got[b])
            toks = got[:2]


def test_cpu_backend_json_rows_follow_the_host_pipeline(C, assets, synth):
    pieces, bos_id, eos = synth
    table = C.JsonTable(pieces, bos_id, eos)
    be = C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)
    with pytest.raises(RuntimeError):
        be.forward_sample([3], [0], [0], [0.8], [0.9], [0.3], logit_procs=[dict(json=True, fresh=True)])
    be.set_json_table(table)
    run_json_rows(be, C, table)


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


BIAS = {str(ord("{")): 10, str(ord('"')): 90, str(ord("}")): 80, str(ord(":")): 70}
JSON = {"type": "json_object"}


def check_bias_driven_object(url):
    """Shared with the GPU test. Every state on the path has one highest-bias allowed token, so the
    reply does not depend on the weights: `{` (the only biased token START allows), `"` (over `}`),
    `"`, `:`, `"`, `"`, `}`, and then only an EOS is allowed."""
    got = _chat(url, PROMPTS[0], 24, logit_bias=BIAS, response_format=JSON)
    choice = got["choices"][0]
    assert choice["message"]["content"] == '{"":""}' and choice["finish_reason"] == "stop"
    assert got["generated_text"] == '{"":""}' and json.loads(got["generated_text"]) == {"": ""}
    plain = _chat(url, PROMPTS[0], 24, logit_bias=BIAS)
    assert plain["generated_text"] != '{"":""}'
    return got


def test_api_bias_driven_reply_is_the_empty_pair(api):
    check_bias_driven_object(api)


def test_api_length_ends_a_valid_prefix(api):
    got = _chat(api, PROMPTS[0], 3, logit_bias=BIAS, response_format=JSON)
    assert got["generated_text"] == '{""' and got["choices"][0]["finish_reason"] == "length"


def test_api_stop_strings_keep_working(api):
    got = _chat(api, PROMPTS[0], 24, logit_bias=BIAS, response_format=JSON, stop=[":"])
    assert got["generated_text"] in ('{""', '{"":') and got["choices"][0]["finish_reason"] == "stop"


def test_api_sampled_stream_stays_a_prefix(api):
    text = b""
    state = PY_START
    finish = None
    for raw in _post(api, PROMPTS[1], 48, stream=True, temperature=0.8, seed=7, response_format=JSON):
        line = raw.decode().strip()
        if not line.startswith("data: ") or line == "data: [DONE]":
            continue
        ch = json.loads(line[6:])["choices"][0]
        finish = ch["finish_reason"] or finish
        delta = ch["delta"].get("content", "")
        if finish:  # (a text cut by `length` inside a character ends in U+FFFD)
            delta = delta.rstrip("�")
        text += delta.encode()
        state = py_walk(delta.encode(), state)
        assert state is not None, text
    assert finish in ("stop", "length") and len(text) >= 1 and text.lstrip(WS)[:1] == b"{"
    if finish == "stop":
        assert py_done(state) and isinstance(json.loads(text), dict)


@pytest.mark.parametrize("bad", [{"type": "json_schema", "json_schema": {"name": "x", "schema": {}}}, {"type": "xml"},
                                 {"type": 3}, {}, "json_object", 1, True, ["json_object"]])
def test_api_response_format_validation(api, bad):
    with pytest.raises(urllib.error.HTTPError) as e:
        _chat(api, PROMPTS[0], response_format=bad)
    assert e.value.code == 400 and "error" in json.loads(e.value.read())


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11)])
def test_api_text_null_and_absent_are_one(api, sampling):
    plain = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, **sampling)
    for rf in ({"type": "text"}, None):
        got = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, response_format=rf, **sampling)
        assert got["generated_text"] == plain["generated_text"] and got["usage"] == plain["usage"]
        assert got["choices"][0]["logprobs"] == plain["choices"][0]["logprobs"]


def test_api_counts_json_requests(api):
    health = lambda: json.loads(urllib.request.urlopen(api + "/health", timeout=10).read())
    before = health()
    _chat(api, PROMPTS[1], 3, response_format=JSON)
    _chat(api, PROMPTS[1], 3, temperature=0.8, response_format=JSON)
    _chat(api, PROMPTS[1], 3, response_format={"type": "text"})
    _chat(api, PROMPTS[1], 3)
    after = health()
    assert after["json_requests"] == before["json_requests"] + 2
    assert after["logit_proc_requests"] == before["logit_proc_requests"]
    text = urllib.request.urlopen(api + "/v1/metrics", timeout=10).read().decode()
    assert "dllama_json_requests_total" in text
