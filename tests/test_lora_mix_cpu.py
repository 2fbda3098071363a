"""Per-row adapter blends on the host side (include/indextts_hip.h): the entry point is declared, exported and bound, the
32-byte record packs as the header lays it out, bad calls are reported without a launch, and GPTEngine.check_adapter_mix accepts
every input form and refuses every bad one before anything reaches the device (no GPU needed: validation comes first)."""
import ctypes
import os
import re
import struct
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_exports_and_binds_the_mix_entry_point():
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_abi_version() == 10
    main = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert re.search(r"#define ITTS_ABI_VERSION (\d+)", main).group(1) == "10"
    txt = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert "itts_lora_shrink_mix" in re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", txt) and "itts_lora_shrink_mix" in nat.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), "itts_lora_shrink_mix")
    assert L.itts_lora_shrink_mix.argtypes is not None and callable(nat.lora_shrink_mix)
    # one argument struct for the id launch and the mix launch (LP64): the header's field order, ids where it was, mix last
    decl = txt[txt.index("typedef struct itts_lora_shrink_args {"):txt.index("} itts_lora_shrink_args;")]
    order = [n for line in decl.split("{", 1)[1].split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert order == [n for n, _ in nat.LoraShrinkArgs._fields_]
    assert (nat.LoraShrinkArgs.ids.offset, nat.LoraShrinkArgs.mix.offset) == (32, 88)
    assert "const itts_lora_shrink_args* a" in txt[txt.index("int itts_lora_shrink_mix("):]


def test_record_layout():
    """32 bytes, entry j = {int32 id; float weight} at byte 8 j, unused entries id -1 -- through pack_lora_mix, the path the engine
    uploads its table with."""
    from indextts import _native as nat
    assert ctypes.sizeof(nat.LoraMixRow) == nat.LORA_MIX_ROW_BYTES == 32 and nat.LORA_MIX_ENTRIES == 4
    assert (nat.LoraMixEntry.id.offset, nat.LoraMixEntry.weight.offset, ctypes.sizeof(nat.LoraMixEntry)) == (0, 4, 8)
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert re.search(r"#define ITTS_LORA_MIX_ENTRIES 4\b", hdr) and "aligned(16)" in hdr
    rows = nat.pack_lora_mix([(), ((2, 1.0),), ((0, 0.7), (1, 0.3)), ((0, 0.5), (1, -0.25), (2, 1.25), (3, 2.0))])
    assert rows.shape == (4, 32) and rows.dtype.name == "uint8"
    got = [struct.unpack("<ifififif", bytes(r)) for r in rows]
    assert got[0] == (-1, 0.0, -1, 0.0, -1, 0.0, -1, 0.0)
    assert got[1] == (2, 1.0, -1, 0.0, -1, 0.0, -1, 0.0)
    assert got[2][:4] == (0, struct.unpack("<f", struct.pack("<f", 0.7))[0], 1, struct.unpack("<f", struct.pack("<f", 0.3))[0])
    assert got[2][4:] == (-1, 0.0, -1, 0.0)
    assert got[3] == (0, 0.5, 1, -0.25, 2, 1.25, 3, 2.0)
    assert nat.pack_lora_mix([]).shape == (0, 32)
    with pytest.raises(ValueError):
        nat.pack_lora_mix([tuple((i, 1.0) for i in range(5))])


def args(nat, **kw):
    a = nat.LoraShrinkArgs()
    a.dtype, a.M, a.K = nat.BF16, 4, 64
    a.x = a.mix = a.a_bank = a.u = 0x1000          # never dereferenced: every call below fails its checks
    a.n, a.rp, a.Kx, a.ldu = 3, 16, 64, 128
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_bad_calls_are_reported_without_launching():
    """The limits and refusals of itts_lora_shrink (tests/test_lora_bank_cpu.py), and the record table's alignment."""
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_lora_shrink_mix(ctypes.byref(nat.LoraShrinkArgs()), None) == 1 and b"null" in L.itts_last_error()
    for kw, word in ((dict(n=0, Kx=0), b"adapters"), (dict(rp=80, Kx=256), b"rank"), (dict(rp=24, Kx=96), b"rp"),
                     (dict(n=9, rp=64, Kx=576), b"Kx"), (dict(Kx=96), b"Kx"), (dict(K=48), b"K %"), (dict(dtype=7), b"dtype"),
                     (dict(ldu=32), b"ldu"), (dict(u=0x1004), b"aligned"), (dict(mix=0x1008), b"aligned"), (dict(x_mtp=1), b"x_mtp"),
                     (dict(mix=0), b"null")):
        assert L.itts_lora_shrink_mix(ctypes.byref(args(nat, **kw)), None) == 1, kw
        assert b"itts_lora_shrink_mix" in L.itts_last_error() and word in L.itts_last_error(), (kw, L.itts_last_error())
    with pytest.raises(nat.NativeError):             # the wrapper wants device tensors: there is no host path
        nat.lora_shrink_mix(torch.zeros(4, 64), torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(1, 16, 64), torch.zeros(4, 32), 4, 64,
                            ldu=32)


def bare_engine(n):
    """A GPTEngine with nothing but a bank of n adapters' shape: all that the host-side checks read."""
    from indextts.gpt.engine import GPTEngine
    eng = object.__new__(GPTEngine)
    eng.bank = None if n is None else SimpleNamespace(n=n, rp=16, Kx=64, sig=(n, 16, ()))
    return eng


def test_check_adapter_mix_accepts_every_form():
    import numpy as np
    eng = bare_engine(3)
    got = eng.check_adapter_mix([None, -1, 2, {0: 0.7, 1: 0.3}, [(2, -0.5), (0, 1.25)], ((1, 0.6),), {}, np.int64(1), {1: 0}], 9)
    assert got == [(), (), ((2, 1.0),), ((0, 0.7), (1, 0.3)), ((0, 1.25), (2, -0.5)), ((1, 0.6),), (), ((1, 1.0),), ((1, 0.0),)]
    assert all(isinstance(w, float) and isinstance(i, int) for row in got for i, w in row)
    assert eng.check_adapter_mix(got, 9) == got                                      # normalised mixes pass unchanged
    assert eng.check_adapter_mix([{0: 1.0, 1: 1.0, 2: 1.0}], 1) == [((0, 1.0), (1, 1.0), (2, 1.0))]
    four = bare_engine(6).check_adapter_mix([{5: 0.25, 1: 0.25, 3: 0.25, 0: 0.25}], 1)
    assert four == [((0, 0.25), (1, 0.25), (3, 0.25), (5, 0.25))]
    assert eng.check_adapter_mix(torch.tensor([0, -1, 2]), 3) == [((0, 1.0),), (), ((2, 1.0),)]
    assert eng._voices([0, 1, -1], None, 3) == ([0, 1, -1], None) and eng._voices(None, None, 2) == ([-1, -1], None)
    assert eng._voices(None, [0, None], 2) == (None, [((0, 1.0),), ()])


@pytest.mark.parametrize("bad", [
    [{6: 1.0}],                                   # id >= n
    [{-1: 1.0}],                                  # an entry's id is never -1: the empty mix is None / -1 / {}
    [-2],                                         # no such id
    [6],
    [[(0, 0.5), (0, 0.5)]],                       # a repeated id within a row
    [{0: float("nan")}],
    [{0: float("inf")}],
    [[(1, float("-inf"))]],
    [{0: "1.0"}],                                 # not a number
    [{0.5: 1.0}],                                 # not an id
    [1.5],
    ["voice"],
    [[0, 1]],                                     # ids without weights
    [{0: .2, 1: .2, 2: .2, 3: .2, 4: .2}],        # more than four entries
], ids=repr)
def test_check_adapter_mix_refuses(bad):
    with pytest.raises(ValueError, match="adapter_mix"):
        bare_engine(6).check_adapter_mix(bad, 1)


def test_check_adapter_mix_refuses_a_wrong_number_of_rows_and_a_missing_bank():
    eng = bare_engine(3)
    for mix, B in (([0, 1], 3), ([0, 1, 2, 0], 3), ([], 1)):
        with pytest.raises(ValueError, match="batch of"):
            eng.check_adapter_mix(mix, B)
    with pytest.raises(ValueError, match="no adapter bank"):
        bare_engine(None).check_adapter_mix([0], 1)
    with pytest.raises(ValueError, match="no adapter bank"):
        bare_engine(None).check_adapter_mix([None], 1)          # even the base mix: a mix is a request for the bank's launch


def test_ids_and_mixes_are_mutually_exclusive():
    """Refused in the first line of prefill() / latent() / latent_mel_rows(), before a buffer is touched."""
    eng = bare_engine(3)
    emb = torch.zeros(2, 3, 64)
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng._voices([0, 1], [0, 1], 2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng.prefill(emb, torch.zeros(2, dtype=torch.int32), 4, adapter_ids=[0, 1], adapter_mix=[0, 1])
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng.latent(emb, adapter_ids=[0, 1], adapter_mix=[{0: 0.5}, None])
    with pytest.raises(ValueError, match="adapter_mix"):       # and a bad mix alone, likewise
        eng.prefill(emb, torch.zeros(2, dtype=torch.int32), 4, adapter_mix=[0, 7])
