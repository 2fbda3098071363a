#!/usr/bin/env python3
"""Generates tests/golden/dvae_small.npz: a small instance of the reference's DiscreteVAE (indextts/vqvae/xtts_dvae.py) run on the
CPU in this container (never on the GPU box), for the tokenizer tests (tests/test_codec_*.py).

DiscreteVAE(channels=100, num_tokens=64, hidden_dim=32, num_resnet_blocks=3, codebook_dim=32, num_layers=2, positional_dims=1,
kernel_size=3, use_transposed_convs=False) under a fixed seed.  Written: the encoder's and the codebook's entries of the state
dict ("sd/<key>"; the decoder half is not used by anything here), and for mels of 1, 2, 3, 4, 5, 37 and 160 frames the mel, z from
the class in fp32, z from the class in .double(), and get_codebook_indices.  The seed is the first one at which every frame is
decided in the sense of tests/codec_refs.py::undecided, so that the tests may require equal codes on every frame.
Only data is written."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_harness as H  # noqa: E402

H.install()
from indextts.vqvae.xtts_dvae import DiscreteVAE  # noqa: E402

import codec_refs as R  # noqa: E402


def make(seed):
    torch.manual_seed(seed)
    m = DiscreteVAE(channels=100, num_tokens=64, hidden_dim=32, num_resnet_blocks=3, codebook_dim=32, num_layers=2, positional_dims=1,
                    kernel_size=3, use_transposed_convs=False).eval()
    out = {"sd/" + k: v.numpy().copy() for k, v in m.state_dict().items() if k.startswith("encoder.") or k == "codebook.embed"}
    md = DiscreteVAE(channels=100, num_tokens=64, hidden_dim=32, num_resnet_blocks=3, codebook_dim=32, num_layers=2, positional_dims=1,
                     kernel_size=3, use_transposed_convs=False).double().eval()
    md.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for T in R.FRAMES:
            mel = (torch.rand(1, 100, T, generator=g) * 8.0 - 6.0)                       # log-mel values: -6 .. 2
            out[f"mel_{T}"] = mel[0].numpy().copy()
            out[f"z32_{T}"] = m.encoder(mel)[0].t().contiguous().numpy()
            out[f"z64_{T}"] = md.encoder(mel.double())[0].t().contiguous().numpy()
            out[f"codes_{T}"] = m.get_codebook_indices(mel)[0].numpy().astype(np.int64)
            assert out[f"codes_{T}"].shape == (R.code_count(T),)
            assert np.array_equal(out[f"codes_{T}"], md.get_codebook_indices(mel.double())[0].numpy())
    return out


for seed in range(100):
    data = make(seed)
    np.savez(R.FIXTURE + ".tmp.npz", **data)
    os.replace(R.FIXTURE + ".tmp.npz", R.FIXTURE)
    fx = R.fixture()
    left = R.undecided(fx)
    print(f"seed {seed}: tau = {R.tau(fx):.3e}, {len(left)} frames undecided")
    if not left:
        break
else:
    raise SystemExit("no seed below 100 decides every frame")
print(f"wrote {R.FIXTURE} ({os.path.getsize(R.FIXTURE)} bytes), seed {seed}")
