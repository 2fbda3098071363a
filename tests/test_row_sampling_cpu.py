"""Per-row sampling settings on the host side (itts_sample_rows, gpt.model.row_sampling_params): the symbol is declared, exported and
bound, a list of settings is checked before anything touches the device, seed and draw stream resolve as
documented, and a record packs as include/indextts_hip.h lays it out (no GPU needed: validation comes first)."""
import ctypes
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = dict(do_sample=True, top_p=0.8, top_k=30, temperature=1.0, repetition_penalty=10.0)


def test_symbol_is_exported_and_reports_bad_calls_without_launching():
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_abi_version() == 10
    # the registry rule of indextts_hip.h: the prototype is declared there, exported by the library and bound by the Python side
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "indextts_hip.h")).read(), flags=re.S)
    assert "itts_sample_rows" in re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", txt) and "itts_sample_rows" in nat.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), "itts_sample_rows")
    # one argument struct for both entry points: the header's field order, `rows` last
    decl = txt[txt.index("typedef struct itts_sample_args {"):txt.index("} itts_sample_args;")]
    order = [n for line in decl.split("{", 1)[1].split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert order == [f[0] for f in nat.SampleArgs._fields_] and order[-1] == "rows"
    a = nat.SampleArgs()
    assert L.itts_sample_rows(ctypes.byref(a), None) == 1 and b"itts_sample_rows: null" in L.itts_last_error()
    a.logits = a.tokens = a.history = a.finished = a.state = 0x1000     # never dereferenced: every call below fails its checks
    a.B, a.V, a.ldl = 2, 9000, 9000
    assert L.itts_sample_rows(ctypes.byref(a), None) == 1 and b"bad shape" in L.itts_last_error()
    a.V, a.ldl = 8194, 8194
    assert L.itts_sample_rows(ctypes.byref(a), None) == 1 and b"rows" in L.itts_last_error()          # no table
    a.rows = 0x1008
    assert L.itts_sample_rows(ctypes.byref(a), None) == 1 and b"16-byte aligned" in L.itts_last_error()
    # the scalar form's refusals are what they were, and it refuses a table (per-row settings are never silently dropped)
    s = nat.SampleArgs()
    assert L.itts_sample(ctypes.byref(s), None) == 1 and b"itts_sample: null pointer" in L.itts_last_error()
    a.rows = 0x1000
    assert L.itts_sample(ctypes.byref(a), None) == 1 and L.itts_last_error().startswith(b"itts_sample: rows")


def test_record_packs_as_the_header_documents_it():
    """The byte offsets are read out of the header's comment, the struct out of its declaration; the binding's record and
    pack_sample_rows agree with both."""
    from indextts import _native as nat
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    doc = hdr[hdr.index("Record: 32 bytes"):hdr.index("typedef struct itts_sample_row {")]
    offs = {name: (int(off), typ) for off, typ, name in re.findall(r"(?:byte)?\s+(\d+)\s+(float|int32|uint32|uint64)\s+(\w+)", doc)}
    assert offs == {"rep_penalty": (0, "float"), "temperature": (4, "float"), "top_p": (8, "float"), "top_k": (12, "int32"),
                    "seed": (16, "uint64"), "stream": (24, "uint32"), "do_sample": (28, "int32")}
    decl = hdr[hdr.index("typedef struct itts_sample_row {"):hdr.index("} itts_sample_row;")]
    order = re.findall(r"(\w+)\s*[,;]", decl.split("{", 1)[1])
    assert order == ["rep_penalty", "temperature", "top_p", "top_k", "seed", "stream", "do_sample"]
    assert ctypes.sizeof(nat.SampleRow) == nat.SAMPLE_ROW_BYTES == 32
    for name, (off, _) in offs.items():
        assert getattr(nat.SampleRow, name).offset == off, name
    rows = [dict(do_sample=True, temperature=0.7, top_k=30, top_p=0.8, repetition_penalty=10.0, seed=(5 << 32) + 7, stream=9),
            dict(do_sample=False, temperature=3.0, top_k=77, top_p=0.1, repetition_penalty=1.5, seed=1, stream=(1 << 32) - 1)]
    raw = nat.pack_sample_rows(rows)
    assert raw.shape == (2, 32) and raw.dtype.name == "uint8"
    fmt = "<fffiQIi"
    assert struct.calcsize(fmt) == 32
    assert struct.unpack(fmt, raw[0].tobytes()) == struct.unpack(fmt, struct.pack(fmt, 10.0, 0.7, 0.8, 30, (5 << 32) + 7, 9, 1))
    # a greedy row ignores the distribution settings: they are normalised (as sampling_params does for the scalar form)
    assert struct.unpack(fmt, raw[1].tobytes()) == (1.5, 1.0, 1.0, 1, 1, (1 << 32) - 1, 0)


def test_seed_and_stream_resolution():
    from indextts.gpt.model import row_sampling_params
    rows = row_sampling_params([{}, None, dict(seed=(1 << 40) + 3), dict(seed=5, stream=11), dict(stream=2, temperature=0.5),
                                dict(do_sample=False, repetition_penalty=2.0)], 6, GEN, 1234)
    assert [r["seed"] for r in rows] == [1234, 1234, (1 << 40) + 3, 5, 1234, 1234]
    # an entry with its own seed draws from stream 0 wherever it sits; one under the call's seed from its utterance's index
    assert [r["stream"] for r in rows] == [0, 1, 0, 11, 2, 5]
    assert rows[0] == dict(GEN, seed=1234, stream=0)
    assert rows[4]["temperature"] == 0.5 and rows[4]["top_k"] == 30 and rows[4]["repetition_penalty"] == 10.0
    assert rows[5]["do_sample"] is False and rows[5]["repetition_penalty"] == 2.0
    assert all(set(r) == {"do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "seed", "stream"} for r in rows)


@pytest.mark.parametrize("bad", [
    dict(top_k=0), dict(top_k=1025), dict(top_k=None), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(temperature=0.0),
    dict(temperature=-1.0), dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0),
    dict(do_sample=False, repetition_penalty=0.0), dict(typical_mass=0.9), dict(num_beams=3), dict(stream=-1), dict(stream=1 << 32)])
def test_a_bad_list_is_refused_on_the_host(bad, monkeypatch):
    """Every refusal is a ValueError raised before the device is touched: the native library is not even loaded."""
    from indextts import _native as nat
    from indextts.gpt.engine import GPTEngine
    from indextts.gpt.model import row_sampling_params

    def no_lib():
        raise AssertionError("validation must not reach the native library")
    monkeypatch.setattr(nat, "lib", no_lib)
    with pytest.raises(ValueError):
        row_sampling_params([{}, bad, {}], 3, GEN, 0)
    row_sampling_params([{}, {}, {}], 3, GEN, 0)                       # (the list is fine without the bad entry)
    full = dict(GEN, seed=0, stream=0)
    if set(bad) <= set(full):                                          # the engine's own check of complete dicts
        with pytest.raises(ValueError):
            GPTEngine.check_row_settings([full, dict(full, **{k: (0 if v is None else v) for k, v in bad.items()})], 2)
    GPTEngine.check_row_settings([full, full], 2)


def test_wrong_length_and_wrong_type_are_refused():
    from indextts.gpt.engine import GPTEngine
    from indextts.gpt.model import row_sampling_params
    for sampling in ([{}, {}], [{}] * 4, {}, None):
        with pytest.raises(ValueError):
            row_sampling_params(sampling, 3, GEN, 0)
    full = dict(GEN, seed=0, stream=0)
    with pytest.raises(ValueError):
        GPTEngine.check_row_settings([full], 2)
    with pytest.raises(ValueError):                                    # the engine takes complete dicts only
        GPTEngine.check_row_settings([full, {k: v for k, v in full.items() if k != "stream"}], 2)
    # greedy rows may carry sampling settings that a sampling row may not: they are ignored, not checked
    assert GPTEngine.check_row_settings([dict(full, do_sample=False, top_k=0, top_p=0.0, temperature=0.0)], 1)[0]["top_k"] == 1
