"""Structured outputs (`response_format: json_schema`) on the CPU backend: the schema compiler
(`Grammar.from_schema`), the host token mask and advance, the CPU backend's rows and `dllama-api`.

Ground truth is not the code under test: a document is valid when `json.loads` parses it and the
small validator below (the supported subset only) accepts the value; the mask's reference is the same
table walk written in numpy (`np_token_walk`), which the GPU tests share."""
import json
import os
import random
import subprocess
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_logprobs import PROMPTS, _chat, _post
from test_prefix_cache import _start_api

F32 = np.float32
NEG_INF = F32(-np.inf)
DEAD = 0xFFFF
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- the validator

def same(a, b):
    return type(a) is type(b) and a == b


def validate(schema, v, root=None):
    root = schema if root is None else root
    if "$ref" in schema:
        return validate(root["$defs"][schema["$ref"].rsplit("/", 1)[1]], v, root)
    if "anyOf" in schema:
        return any(validate(s, v, root) for s in schema["anyOf"])
    if "const" in schema:
        return same(v, schema["const"])
    if "enum" in schema:
        return any(same(v, e) for e in schema["enum"])
    types = schema["type"] if isinstance(schema["type"], list) else [schema["type"]]
    return any(_typed(t, schema, v, root) for t in types)


def _typed(t, schema, v, root):
    if t == "string":
        return isinstance(v, str) and schema.get("minLength", 0) <= len(v) <= schema.get("maxLength", 1 << 30)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "boolean":
        return isinstance(v, bool)
    if t == "null":
        return v is None
    if t == "object":
        props = schema["properties"]
        return isinstance(v, dict) and list(v) == list(props) and all(validate(props[k], v[k], root) for k in props)
    assert t == "array"
    return (isinstance(v, list) and schema.get("minItems", 0) <= len(v) <= schema.get("maxItems", 1 << 30)
            and all(validate(schema["items"], x, root) for x in v))


def valid_document(schema, data: bytes) -> bool:
    try:
        return validate(schema, json.loads(data.decode("utf-8")))
    except ValueError:
        return False


def obj(props, **kw):
    return dict(type="object", properties=props, required=list(props), additionalProperties=False, **kw)


# ---------------------------------------------------------------------------- schemas and documents
# name -> (schema, accepted documents, rejected documents)

POINT = obj({"x": {"type": "number"}, "y": {"type": "number"}})
CASES = {
    "flat": (obj({"s": {"type": "string"}, "n": {"type": "number"}, "i": {"type": "integer"}, "b": {"type": "boolean"},
                  "z": {"type": "null"}}),
             [b'{"s":"","n":0,"i":0,"b":true,"z":null}',
              b'{"s": "a\\n\\u00e9\xe6\x97\xa5 \\"q\\"", "n": -1.5e+10, "i": -12, "b": false, "z": null}',
              b'{"s":"x","n":1E5,"i":7,"b":true,"z":null}'],
             [b'{"s":"","n":0,"i":0.5,"b":true,"z":null}', b'{"s":"","n":01,"i":0,"b":true,"z":null}',
              b'{"s":"","n":0,"i":0,"b":1,"z":null}', b'{"s":"\xff","n":0,"i":0,"b":true,"z":null}',
              b'{"s":"\\x","n":0,"i":0,"b":true,"z":null}', b'{"s":"","n":0,"i":0,"b":true,"z":null} ',
              b'{"s":"","n":-,"i":0,"b":true,"z":null}', b'{"s":"","n":1.,"i":0,"b":true,"z":null}']),
    "nested": (obj({"a": obj({"b": obj({"c": {"type": "integer"}}), "d": obj({})}), "e": {"type": "boolean"}}),
               [b'{"a":{"b":{"c":1},"d":{}},"e":true}', b'{"a": {"b": {"c": -3}, "d": {}}, "e": false}'],
               [b'{"a":{"b":{"c":1},"d":{"x":1}},"e":true}', b'{"a":{"b":{},"d":{}},"e":true}', b'{"a":{"b":{"c":1},"d":{}}}']),
    "array": (obj({"l": {"type": "array", "items": obj({"x": {"type": "integer"}}), "minItems": 1, "maxItems": 3}}),
              [b'{"l":[{"x":1}]}', b'{"l":[{"x":1}, {"x":2},{"x":3}]}'],
              [b'{"l":[]}', b'{"l":[{"x":1},{"x":2},{"x":3},{"x":4}]}', b'{"l":[{"x":1},]}', b'{"l":[{"x":"1"}]}']),
    "enum": (obj({"e": {"enum": ['say "hi"\\', "été\n", "plain"]}, "c": {"const": "k"}, "t": {"enum": [True, None]}}),
             [b'{"e":"say \\"hi\\"\\\\","c":"k","t":true}', b'{"e":"\xc3\xa9t\xc3\xa9\\u000a","c":"k","t":null}',
              b'{"e": "plain", "c": "k", "t": null}'],
             [b'{"e":"\xc3\xa9t\xc3\xa9\\n","c":"k","t":true}', b'{"e":"\\u00e9t\\u00e9\\u000a","c":"k","t":true}',
              b'{"e":"plai","c":"k","t":true}', b'{"e":"plain","c":"K","t":true}', b'{"e":"plain","c":"k","t":false}']),
    "anyof": (obj({"v": {"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 2},
                                   {"type": "array", "items": {"type": "null"}, "maxItems": 2}]}}),
              [b'{"v":12}', b'{"v":"ab"}', b'{"v":[]}', b'{"v":[null, null]}'],
              [b'{"v":1.5}', b'{"v":"abc"}', b'{"v":[null,null,null]}', b'{"v":true}']),
    "nullable": (obj({"v": {"type": ["string", "null"]}, "w": {"type": ["integer", "boolean"]}}),
                 [b'{"v":null,"w":1}', b'{"v":"null","w":false}'], [b'{"v":1,"w":1}', b'{"v":null,"w":null}', b'{"v":nul,"w":1}']),
    "ref": (dict(obj({"a": {"$ref": "#/$defs/p"}, "b": {"type": "array", "items": {"$ref": "#/$defs/p"}, "maxItems": 2}}),
                 **{"$defs": {"p": POINT}}),
            [b'{"a":{"x":1,"y":2.5},"b":[]}', b'{"a":{"x":0,"y":0},"b":[{"x":1e3,"y":-1}]}'],
            [b'{"a":{"y":1,"x":2},"b":[]}', b'{"a":{"x":1},"b":[]}', b'{"a":{"x":1,"y":2,"z":3},"b":[]}']),
    "length": (obj({"s": {"type": "string", "minLength": 2, "maxLength": 4}}),
               [b'{"s":"ab"}', b'{"s":"\xc3\xa9\\u00e9\xf0\x9f\x98\x80\\n"}', b'{"s":"abcd"}'],
               [b'{"s":"a"}', b'{"s":"abcde"}', b'{"s":""}', b'{"s":"a\xc3"}']),
    "unbounded": (obj({"l": {"type": "array", "items": {"type": "boolean"}, "minItems": 2}}),
                  [b'{"l":[true,false]}', b'{"l":[true, false,true,true,true,true,true,true,true,true,true,true,true,true,true,true,true,true]}'],
                  [b'{"l":[true]}', b'{"l":[]}', b'{"l":[true,false,]}']),
    "empty": (obj({}), [b"{}"], [b"{ }", b'{"a":1}', b"{}{}", b""]),
    "finite": (obj({"kind": {"enum": ["cat", "dog"]}, "ok": {"type": "boolean"}, "v": {"const": 1}, "z": {"type": "null"},
                    "tags": {"type": "array", "items": {"enum": ["a", "b"]}, "maxItems": 2}}),
               [b'{"kind":"cat","ok":true,"v":1,"z":null,"tags":[]}', b'{"kind": "dog", "ok": false, "v": 1, "z": null, "tags": ["a", "b"]}'],
               [b'{"kind":"cow","ok":true,"v":1,"z":null,"tags":[]}', b'{"kind":"cat","ok":true,"v":2,"z":null,"tags":[]}',
                b'{"kind":"cat","ok":true,"v":1,"z":null,"tags":["a","b","a"]}']),
}
# numbers are spelled as the schema's text spells them: the text is written by hand
NUMBER_ENUM_TEXT = '{"type":"object","properties":{"n":{"enum":[1,2.50,-3e2]},"m":{"type":"integer","enum":[4,4.5]}},"required":["n","m"]}'
FINITE = CASES["finite"][0]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    from distributed_llama_multiusers_amd.models.synthetic import make_tokenizer
    info = make_tokenizer(str(tmp_path_factory.mktemp("schema_tok") / "t.t"), 512)
    return info["tokens"], info["bos_id"], info["eos"]


@pytest.fixture(scope="module")
def table(C, synth):
    return C.JsonTable(*synth)


def compile_case(C, name, table=None):
    return C.Grammar.from_schema(json.dumps(CASES[name][0]), table)


# ---------------------------------------------------------------------------- compiler semantics

@pytest.mark.parametrize("name", list(CASES))
def test_accepted_and_rejected_documents(C, table, name):
    schema, good, bad = CASES[name]
    g = compile_case(C, name, table)
    assert 1 <= g.n_states <= 4096 and 1 <= g.n_classes <= 256 and g.n_states * g.n_classes <= 131072
    for d in good:
        assert valid_document(schema, d), d  # (the test's own documents are what they claim to be)
        assert g.accepts(d), d
        for cut in range(len(d)):  # every prefix is live, none but the whole accepts
            s = g.walk(d[:cut])
            assert s is not None and not g.is_accepting(s), (d, cut)
    for d in bad:
        assert not g.accepts(d), d


def outside_strings(d: bytes):
    """positions i of d such that an insertion in front of d[i] (or at the end) lies outside every string"""
    out, inside, esc = [], False, False
    for i, c in enumerate(d):
        if not inside:
            out.append(i)
        if inside and esc:
            esc = False
        elif inside and c == 0x5C:
            esc = True
        elif c == 0x22:
            inside = not inside
    return out + [len(d)]


@pytest.mark.parametrize("name", list(CASES))
def test_whitespace_only_behind_colon_and_comma(C, name):
    g = compile_case(C, name)
    for d in CASES[name][1]:
        for i in outside_strings(d):
            for ws in (b" ", b"\n", b"\t", b"\r"):
                allowed = ws == b" " and i > 0 and d[i - 1:i] in (b":", b",") and d[i:i + 1] != b" "
                assert g.accepts(d[:i] + ws + d[i:]) == allowed, (d, i, ws)


def compact(v):
    return json.dumps(v, separators=(",", ":"), ensure_ascii=False).encode()


@pytest.mark.parametrize("name", ["flat", "nested", "array", "ref", "finite", "nullable"])
def test_key_order_missing_extra_and_wrong_type_reject(C, name):
    schema, good, _ = CASES[name]
    g = compile_case(C, name)
    wrong = {str: 1, int: "1", float: "1", bool: "x", type(None): 0, dict: [], list: {}}
    tried = 0
    for d in good:
        v = json.loads(d)
        assert g.accepts(compact(v)) or name == "enum"

        def variants(node, rebuild):
            if isinstance(node, dict):
                keys = list(node)
                if len(keys) >= 2:
                    yield rebuild({k: node[k] for k in [keys[1], keys[0]] + keys[2:]})
                if keys:
                    yield rebuild({k: node[k] for k in keys[1:]})
                yield rebuild(dict(node, extra=1))
                for k in keys:
                    yield rebuild(dict(node, **{k: wrong[type(node[k])]}))
                    yield from variants(node[k], lambda x, k=k: rebuild(dict(node, **{k: x})))
            elif isinstance(node, list):
                for i in range(len(node)):
                    yield from variants(node[i], lambda x, i=i: rebuild(node[:i] + [x] + node[i + 1:]))

        for m in variants(v, lambda x: x):
            if not validate(schema, m):  # (an integer for a number is still valid, and the like)
                assert not g.accepts(compact(m)), m
                tried += 1
    assert tried >= 4


def test_numbers_are_spelled_as_the_schema_spells_them(C):
    g = C.Grammar.from_schema(NUMBER_ENUM_TEXT)
    for n in (b"1", b"2.50", b"-3e2"):
        assert g.accepts(b'{"n":' + n + b',"m":4}')
    for n in (b"1.0", b"2.5", b"-300", b"-3E2", b"2.500"):
        assert not g.accepts(b'{"n":' + n + b',"m":4}')
    assert not g.accepts(b'{"n":1,"m":4.5}')  # 4.5 is no integer: the type filters the enum


# ---------------------------------------------------------------------------- the walk in numpy

class NpVocab:
    """The vocabulary's pieces as a padded byte matrix (built once per vocabulary)."""

    def __init__(self, pieces, bos_id, eos):
        self.n = len(pieces)
        self.lens = np.array([len(p) for p in pieces], np.int64)
        self.mat = np.zeros((self.n, max(int(self.lens.max()), 1)), np.uint8)
        for t, p in enumerate(pieces):
            self.mat[t, :len(p)] = np.frombuffer(p, np.uint8)
        ids = np.arange(self.n)
        self.eos = np.isin(ids, eos)
        self.regular = (ids < bos_id) & ~self.eos


def np_token_walk(tables, state, vocab: NpVocab):
    """(allowed[vocab], state behind each allowed token) by the rules of grammarStepToken."""
    class_of, nxt, _, accept = tables
    nxt = np.asarray(nxt)
    if state >= nxt.shape[0]:
        return np.zeros(vocab.n, bool), np.full(vocab.n, state, np.int64)
    s = np.full(vocab.n, state, np.int64)
    dead = np.zeros(vocab.n, bool)
    for i in range(vocab.mat.shape[1]):
        act = (i < vocab.lens) & ~dead
        if not act.any():
            break
        n = nxt[np.where(act, s, 0), np.asarray(class_of)[vocab.mat[:, i]]].astype(np.int64)
        dead |= act & (n == DEAD)
        s = np.where(act & (n != DEAD), n, s)
    allowed = vocab.regular & (vocab.lens > 0) & ~dead
    allowed |= vocab.eos & (state in accept)
    return allowed, np.where(vocab.eos, state, s)


def np_mask(x, tables, state, vocab):
    return np.where(np_token_walk(tables, state, vocab)[0], x, NEG_INF).astype(F32)


def odd_logits(rng, n):
    x = (np.round(rng.standard_normal(n) * 24) / 4).astype(F32)
    x[rng.integers(0, n, 6)] = [NEG_INF, F32(-0.0), F32(0.0), F32(np.nan), F32(3e38), F32(1e-42)]
    return x


NAMED_PREFIXES = {  # of the "flat" schema: the states the GPU tests name
    "start": b"", "key": b'{"', "string": b'{"s":"ab', "escape": b'{"s":"ab\\', "utf8": b'{"s":"\xe6\x97',
    "number": b'{"s":"","n":-1.5', "done": b'{"s":"","n":0,"i":0,"b":true,"z":null}',
}


def test_host_mask_and_advance_match_the_numpy_walk(C, synth, table):
    vocab = NpVocab(*synth)
    rng = np.random.default_rng(2)
    g = compile_case(C, "flat", table)
    tables = g.tables()
    for name, prefix in NAMED_PREFIXES.items():
        state = g.walk(prefix)
        assert state is not None, name
        x = odd_logits(rng, vocab.n)
        allowed, nxt = np_token_walk(tables, state, vocab)
        assert g.mask_host(x, state).tobytes() == np.where(allowed, x, NEG_INF).astype(F32).tobytes(), name
        assert 1 <= allowed.sum() < vocab.n, name
        assert allowed[vocab.eos].all() == (name == "done") and not allowed[~vocab.regular & ~vocab.eos].any()
        for t in list(rng.integers(0, vocab.n, 40)) + list(np.flatnonzero(allowed)[:20]) + [-1, vocab.n]:
            want = int(nxt[t]) if 0 <= t < vocab.n and allowed[t] else state
            assert g.advance_host(state, int(t)) == want, (name, t)
            if 0 <= t < vocab.n and allowed[t] and not vocab.eos[t]:
                assert want == g.walk(synth[0][t], state)


def edge_dfas(C, table, seed=9):
    """Random raw tables: (name, grammar). Edges: one class, 256 classes, the state cap, the start as
    the last state, an accepting state with outgoing transitions."""
    rng = np.random.default_rng(seed)
    out = []
    for name, n_states, n_classes in (("one_class", 7, 1), ("all_classes", 96, 256), ("state_cap", 4096, 32), ("small", 5, 11)):
        nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(np.uint16)
        nxt[rng.random((n_states, n_classes)) < (0.1 if n_classes == 1 else 0.6)] = DEAD
        class_of = (rng.permutation(256) % n_classes).astype(np.uint8)
        start = n_states - 1
        nxt[start, : max(1, n_classes // 2)] = rng.integers(0, n_states, max(1, n_classes // 2))  # (the start goes somewhere)
        accept = sorted({start, 0, n_states // 2})  # accepting states that keep their transitions
        out.append((name, C.Grammar.from_table(class_of, nxt, start, accept, table)))
    return out


def test_from_table_edges_on_the_host(C, synth, table):
    vocab = NpVocab(*synth)
    rng = np.random.default_rng(4)
    for name, g in edge_dfas(C, table):
        class_of, nxt, start, accept = g.tables()
        assert start == g.n_states - 1 == g.start and g.is_accepting(start)
        for state in (start, 0, g.n_states // 2, int(rng.integers(0, g.n_states))):
            x = odd_logits(rng, vocab.n)
            assert g.mask_host(x, state).tobytes() == np_mask(x, g.tables(), state, vocab).tobytes(), (name, state)
        assert not np.isfinite(g.mask_host(np.zeros(vocab.n, F32), g.n_states)).any()  # no state, no token
    with pytest.raises(RuntimeError):
        C.Grammar.from_table(np.zeros(256, np.uint8), np.full((3, 2), 3, np.uint16), 0, [0])  # next names state 3 of 3
    with pytest.raises(RuntimeError):
        C.Grammar.from_table(np.zeros(256, np.uint8), np.zeros((4097, 1), np.uint16), 0, [0])
    with pytest.raises(RuntimeError):
        C.Grammar.from_table(np.full(256, 2, np.uint8), np.zeros((3, 2), np.uint16), 0, [0])


# ---------------------------------------------------------------------------- random walks

def distance_to_accept(tables):
    _, nxt, _, accept = tables
    nxt = np.asarray(nxt).astype(np.int64)
    dist = np.full(nxt.shape[0], 1 << 30)
    dist[list(accept)] = 0
    for _ in range(nxt.shape[0]):
        via = np.where(nxt == DEAD, 1 << 30, dist[np.minimum(nxt, nxt.shape[0] - 1)]).min(axis=1) + 1
        new = np.minimum(dist, via)
        if (new == dist).all():
            break
        dist = new
    return dist


@pytest.mark.parametrize("name", list(CASES))
def test_random_walks_end_in_valid_documents(C, synth, table, name):
    pieces, bos_id, eos = synth
    schema = CASES[name][0]
    g = compile_case(C, name, table)
    dist = distance_to_accept(g.tables())
    assert dist.max() < 1 << 30  # trimmed: every state reaches an accepting one
    rng = random.Random(sum(name.encode()))
    zeros = np.zeros(len(pieces), F32)
    for walk in range(6):
        state, text = g.start, b""
        for step in range(400):
            allowed = np.flatnonzero(np.isfinite(g.mask_host(zeros, state)))
            assert len(allowed) >= 1
            if any(t in eos for t in allowed):
                assert g.is_accepting(state)
                break
            if step >= 40:  # head for the end: the allowed tokens that come closest to it
                after = [dist[g.advance_host(state, int(t))] for t in allowed]
                allowed = [t for t, d in zip(allowed, after) if d == min(after)]
            t = int(rng.choice(list(allowed)))
            text += pieces[t]
            state = g.advance_host(state, t)
        else:
            raise AssertionError("the walk did not end: " + repr(text))
        assert valid_document(schema, text) and g.accepts(text), text


# ---------------------------------------------------------------------------- refusals

REFUSED = [(k, obj({"a": dict({"type": "string"}, **{k: v})})) for k, v in [
    ("pattern", "^a"), ("format", "date"), ("minimum", 0), ("maximum", 1), ("oneOf", [{"type": "null"}]),
    ("allOf", [{"type": "null"}]), ("not", {"type": "null"}), ("patternProperties", {}), ("uniqueItems", True),
    ("multipleOf", 2), ("exclusiveMinimum", 0), ("if", {}), ("prefixItems", []), ("minProperties", 1)]] + [
    ("additionalProperties", dict(obj({"a": {"type": "null"}}), additionalProperties=True)),
    ("required", dict(obj({"a": {"type": "null"}, "b": {"type": "null"}}), required=["a"])),
    ("properties", {"type": "object"}),
    ("properties", obj({"a": {"type": "object"}})),
    ("any value", obj({"a": {}})),
    ("any value", obj({"a": {"description": "anything"}})),
    ("items", obj({"a": {"type": "array"}})),
    ("maxItems", obj({"a": {"type": "array", "items": {"type": "null"}, "maxItems": 17}})),
    ("minItems", obj({"a": {"type": "array", "items": {"type": "null"}, "minItems": 3, "maxItems": 2}})),
    ("maxLength", obj({"a": {"type": "string", "maxLength": 65}})),
    ("minLength", obj({"a": {"type": "string", "minLength": -1}})),
    ("recursive", dict(obj({"r": {"$ref": "#/$defs/r"}}), **{"$defs": {"r": obj({"r": {"$ref": "#/$defs/r"}})}})),
    ("unknown definition", obj({"r": {"$ref": "#/$defs/nope"}})),
    ("$ref", obj({"r": {"$ref": "http://example.com/x"}})),
    ("top level", {"type": "array", "items": {"type": "null"}}),
    ("top level", {"type": ["object", "null"], "properties": {}}),
    ("top level", {"anyOf": [obj({})]}),
    ("scalar", obj({"a": {"enum": [[1]]}})),
    ("'type'", obj({"a": {"type": "float"}})),
    ("anyOf", obj({"a": {"anyOf": []}})),
]


@pytest.mark.parametrize("word,schema", REFUSED, ids=[f"{i}-{w}" for i, (w, _) in enumerate(REFUSED)])
def test_refusals_name_the_keyword_or_the_reason(C, word, schema):
    with pytest.raises(C.SchemaError) as e:
        C.Grammar.from_schema(json.dumps(schema))
    assert word in str(e.value), str(e.value)


def blow_up(depth):
    s = {"type": "string", "maxLength": 64}
    for _ in range(depth):
        s = {"type": "array", "maxItems": 16, "items": {"anyOf": [s, {"type": "integer"}]}}
    return obj({"a": s})


CAPS = [
    ("NFA states", blow_up(4)),  # 16^4 copies of a 64-code-point string
    ("DFA states", obj({"a": {"type": "array", "minItems": 16, "maxItems": 16, "items": {"type": "string", "minLength": 30, "maxLength": 30}}})),
    ("table entries", obj({"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-+=!@#$%^&*()<>?;|~":
                           {"type": "array", "minItems": 9, "maxItems": 9, "items": {"type": "string", "minLength": 30, "maxLength": 30}}})),
]


@pytest.mark.parametrize("cap,schema", CAPS, ids=[c for c, _ in CAPS])
def test_each_cap_refuses_by_name(C, cap, schema):
    with pytest.raises(C.SchemaError) as e:
        C.Grammar.from_schema(json.dumps(schema))
    assert cap in str(e.value) and "cap" in str(e.value), str(e.value)


def test_dead_end_check_with_a_vocabulary_lacking_the_quote(C, synth):
    pieces, bos_id, eos = synth
    no_quote = [p if p != b'"' else b"" for p in pieces]
    with pytest.raises(C.SchemaError) as e:
        C.Grammar.from_schema(json.dumps(CASES["flat"][0]), C.JsonTable(no_quote, bos_id, eos))
    assert "dead end" in str(e.value)
    with pytest.raises(C.SchemaError) as e:
        C.Grammar.from_schema(json.dumps(CASES["empty"][0]), C.JsonTable(pieces, bos_id, []))
    assert "dead end" in str(e.value) and "EOS" in str(e.value)
    C.Grammar.from_schema(json.dumps(CASES["empty"][0]), C.JsonTable(no_quote, bos_id, eos))  # `{}` needs no quote


def test_compiling_is_deterministic_also_through_the_cache(C, table):
    for name in CASES:
        text = json.dumps(CASES[name][0])
        a, b = C.Grammar.from_schema(text, table), C.Grammar.from_schema(text)
        assert a.table_bytes() == b.table_bytes() and not a.same_object(b)
        before = C.schema_cache_stats()
        c, d = C.Grammar.from_schema(text, table, cache=True), C.Grammar.from_schema(text, table, cache=True)
        assert c.same_object(d) and c.table_bytes() == a.table_bytes()
        assert C.schema_cache_stats()[1] >= before[1] + 1
    assert C.schema_cache_stats()[0] <= 32
    # numbers that differ in spelling only are different schemas to the cache
    one = C.Grammar.from_schema(NUMBER_ENUM_TEXT, cache=True)
    other = C.Grammar.from_schema(NUMBER_ENUM_TEXT.replace("2.50", "2.5"), cache=True)
    assert not one.same_object(other) and one.table_bytes() != other.table_bytes()


# ---------------------------------------------------------------------------- Backend.forward_sample

def run_grammar_rows(be, C, table, steps=6, captured=None):
    """Shared with the GPU test. Two requests per slot, the second with other schemas in the same
    slots (a slot must never see the earlier tables): row 0 greedy with penalties, row 1 sampled with
    a bias and top_k 3, row 2 plain. Every constrained draw equals the host pipeline (penalties and
    bias, mask, filter, draw) on `forward`'s own logits, in the state the earlier draws led to."""
    vocab = table.vocab
    names = [("flat", "finite"), ("array", "flat")]
    for request in range(2):
        gs = [compile_case(C, n, table) for n in names[request]]
        states = [g.start for g in gs]
        counts = np.zeros(vocab, np.uint32)
        toks = [65 + request, 66]
        for s in range(steps):
            args = (toks + [67], [s, s, s], [0, 1, 2])
            temps, topps, coins = [0.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.0, (0.17 + 0.29 * s) % 1, 0.5]
            raw = be.forward(*args)
            procs = [dict(grammar=gs[0], fresh=s == 0, presence=0.5, frequency=0.25),
                     dict(grammar=gs[1], fresh=s == 0, top_k=3, bias={34: 5.0}), None]
            got = be.forward_sample(*args, temps, topps, coins, logit_procs=procs)
            assert got[2] == be.forward_sample(*args, temps, topps, coins)[2]
            row0 = C.cpu_ops.logit_proc_host(raw[0], counts, 0.5, 0.25, [], [])
            row1 = C.cpu_ops.logit_proc_host(raw[1], np.zeros(vocab, np.uint32), 0.0, 0.0, [34], [5.0])
            row1 = C.cpu_ops.logit_filter_host(gs[1].mask_host(row1, states[1]), 3, float("-inf"))
            want = [C.cpu_ops.sample_host(gs[0].mask_host(row0, states[0]), 0.0, 0.9, 0.0),
                    C.cpu_ops.sample_host(row1, temps[1], topps[1], coins[1])]
            assert got[:2] == want, (request, s)
            counts[got[0]] += 1
            for b in range(2):
                assert gs[b].mask_host(np.zeros(vocab, F32), states[b])[got[b]] == 0  # the draw was allowed
                states[b] = gs[b].advance_host(states[b], got[b])
            toks = got[:2]


def test_cpu_backend_grammar_rows_follow_the_host_pipeline(C, assets, synth, table):
    be = C.cpu_backend(assets["q40"], "q80", 2, 128, 64, 3)
    g = compile_case(C, "flat", table)
    with pytest.raises(RuntimeError):  # no token table yet
        be.forward_sample([3], [0], [0], [0.8], [0.9], [0.3], logit_procs=[dict(grammar=g, fresh=True)])
    be.set_json_table(table)
    with pytest.raises(RuntimeError):  # a row is in JSON mode or follows a grammar
        be.forward_sample([3], [0], [0], [0.8], [0.9], [0.3], logit_procs=[dict(grammar=g, json=True, fresh=True)])
    run_grammar_rows(be, C, table)
    with pytest.raises(RuntimeError):  # a row that is not fresh cannot change its slot's grammar
        be.forward_sample([3], [7], [0], [0.8], [0.9], [0.3], logit_procs=[dict(grammar=g, fresh=False)])


# ---------------------------------------------------------------------------- dllama-api

@pytest.fixture(scope="module")
def api(assets):
    proc, url = _start_api(assets["q40"], assets["tok"])
    yield url
    proc.kill()
    proc.wait()


def schema_format(schema, **kw):
    return {"type": "json_schema", "json_schema": dict({"name": "reply", "schema": schema, "strict": True}, **kw)}


SAMPLINGS = [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11), dict(temperature=1.3, seed=5, top_k=4, presence_penalty=0.4)]


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_api_finite_schema_ends_with_stop_and_validates(api, sampling):
    got = _chat(api, PROMPTS[0], 100, response_format=schema_format(FINITE), **sampling)
    text = got["generated_text"]
    assert got["choices"][0]["finish_reason"] == "stop" and got["choices"][0]["message"]["content"] == text
    assert valid_document(FINITE, text.encode()), text


def test_api_length_leaves_a_live_prefix(api, C):
    g = C.Grammar.from_schema(json.dumps(FINITE))
    for n in (1, 4, 9):
        got = _chat(api, PROMPTS[1], n, response_format=schema_format(FINITE))
        assert got["choices"][0]["finish_reason"] == "length"
        state = g.walk(got["generated_text"].encode())
        assert state is not None and not g.is_accepting(state)


def test_api_streaming_stays_inside_the_schema(api, C):
    g = C.Grammar.from_schema(json.dumps(FINITE))
    text, finish, state = b"", None, g.start
    for raw in _post(api, PROMPTS[1], 100, stream=True, temperature=0.8, seed=7, response_format=schema_format(FINITE)):
        line = raw.decode().strip()
        if not line.startswith("data: ") or line == "data: [DONE]":
            continue
        ch = json.loads(line[6:])["choices"][0]
        finish = ch["finish_reason"] or finish
        delta = ch["delta"].get("content", "").encode()
        text += delta
        state = g.walk(delta, state)
        assert state is not None, text
    assert finish == "stop" and valid_document(FINITE, text), text


def _complete(url, **body):
    req = urllib.request.Request(url + "/v1/completions", data=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
    return json.loads(urllib.request.urlopen(req, timeout=60).read())


def test_api_completions_takes_the_field(api):
    got = _complete(api, prompt=PROMPTS[2], max_tokens=100, temperature=0, response_format=schema_format(FINITE))
    assert got["choices"][0]["finish_reason"] == "stop" and valid_document(FINITE, got["choices"][0]["text"].encode())


BAD_FORMATS = [
    ("pattern", schema_format(obj({"a": {"type": "string", "pattern": "x"}}))),
    ("top level", schema_format({"type": "array", "items": {"type": "null"}})),
    ("recursive", schema_format(REFUSED[25][1])),
    ("NFA states", schema_format(blow_up(4))),
    ("schema", {"type": "json_schema"}),
    ("schema", {"type": "json_schema", "json_schema": {"name": "x"}}),
    ("schema", {"type": "json_schema", "json_schema": {"name": "x", "schema": "{}"}}),
    ("name", schema_format(FINITE, name=3)),
    ("strict", schema_format(FINITE, strict="yes")),
    ("extra", schema_format(FINITE, extra=1)),
]


@pytest.mark.parametrize("word,rf", BAD_FORMATS, ids=[f"{i}-{w}" for i, (w, _) in enumerate(BAD_FORMATS)])
def test_api_validation_answers_400_and_names_the_reason(api, word, rf):
    assert REFUSED[25][0] == "recursive"
    with pytest.raises(urllib.error.HTTPError) as e:
        _chat(api, PROMPTS[0], response_format=rf)
    assert e.value.code == 400 and word in json.loads(e.value.read())["error"]


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, top_p=0.8, seed=11)])
def test_api_other_formats_are_served_as_before(api, sampling):
    plain = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, **sampling)
    _chat(api, PROMPTS[0], 30, response_format=schema_format(FINITE), **sampling)  # (a schema request in between)
    for rf in ({"type": "text"}, None):
        got = _chat(api, PROMPTS[0], 16, logprobs=True, top_logprobs=3, response_format=rf, **sampling)
        assert got["generated_text"] == plain["generated_text"] and got["usage"] == plain["usage"]
        assert got["choices"][0]["logprobs"] == plain["choices"][0]["logprobs"]
    from test_json_mode import check_bias_driven_object
    check_bias_driven_object(api)


def test_api_logprobs_score_the_raw_logits(api):
    plain = _chat(api, PROMPTS[0], 1, logprobs=True, top_logprobs=5)
    got = _chat(api, PROMPTS[0], 1, logprobs=True, top_logprobs=5, response_format=schema_format(FINITE))
    assert got["generated_text"] == "{"
    top = lambda d: d["choices"][0]["logprobs"]["content"][0]["top_logprobs"]
    assert top(got) == top(plain)  # the candidates are the unmasked row's


def test_api_counts_schema_requests(api):
    health = lambda: json.loads(urllib.request.urlopen(api + "/health", timeout=10).read())
    before = health()
    _chat(api, PROMPTS[1], 3, response_format=schema_format(FINITE))
    _chat(api, PROMPTS[1], 3, temperature=0.8, response_format=schema_format(CASES["flat"][0]))
    _chat(api, PROMPTS[1], 3, response_format={"type": "json_object"})
    _chat(api, PROMPTS[1], 3)
    after = health()
    assert after["schema_requests"] == before["schema_requests"] + 2
    assert after["json_requests"] == before["json_requests"] + 1
    assert after["logit_proc_requests"] == before["logit_proc_requests"]
    text = urllib.request.urlopen(api + "/v1/metrics", timeout=10).read().decode()
    assert "dllama_schema_requests_total" in text and "dllama_json_requests_total" in text


# ---------------------------------------------------------------------------- the sanitizer program

def test_schema_fuzz_program_runs_clean_under_the_host_sanitizers():
    """The compiler parses text from the network: a stand-alone program (its own main, host code only)
    feeds it the schemas and fixed-seed mutations under AddressSanitizer and UBSan."""
    build = subprocess.run(["make", "build/schema_fuzz"], cwd=REPO, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([os.path.join(REPO, "build", "schema_fuzz")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "compiled" in run.stdout, run.stdout + run.stderr
