"""Voice extraction: the LoRA a MERGED fine-tuned checkpoint holds, recovered as factor pairs.

The reference only ever saves merged weights (train.py:802-832: merge_and_unload(), one gpt_finetuned.pth, fp16 by default), so for
each of the 4 x layers target matrices  W_ft - W_base = s A^T B^T + (rounding of the save dtype):  rank r plus full-rank noise far
below it.  A randomised range finder with one power iteration recovers the rank-r part.  The difference D is reached only through
products  D X  and  D^T X  with c-wide blocks -- on the device one launch each of ittv_delta_project (indextts/_native_voice.py),
which forms D in registers from the two checkpoints' own bytes: no [K, N] difference is ever written, and the fine-tuned tensors
are uploaded target by target.  QR and SVD run on c-wide matrices on the host, in float64 (plumbing, not hot path).

    c = 16 ceil(max_rank / 16) + 16;  Omega [N, c] standard normal from a seeded CPU generator (the same on every device)
    Q = orth(D Omega);  Q = orth(D^T Q);  Q = orth(D Q);  Bt = D^T Q;  svd(Bt^T) = U S V^T           (D ~ Q U S V^T)
    r = the index of the largest ratio S_i / S_{i+1}, accepted if that ratio is at least `gap`
    A = (Q U_r sqrt(S_r))^T [r, K],  B = V_r sqrt(S_r) [N, r],  scaling 1.0:  the attach_lora format

What is not a plain rank-r difference is refused (ValueError), before any launch where the state dicts alone show it."""
from __future__ import annotations

import torch

TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")


def target_keys(layers: int):
    return [f"gpt.h.{i}.{name}" for i in range(layers) for name in TARGETS]


def probe_width(max_rank: int) -> int:
    return 16 * ((int(max_rank) + 15) // 16) + 16


def draw_omega(N: int, c: int, seed: int, index: int) -> torch.Tensor:
    """The probe of target number `index`: fp32 [N, c], drawn on the CPU (a generator of its own per target, so a target's result
    does not depend on which other targets changed)."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(index))
    return torch.randn(N, c, generator=g, dtype=torch.float32)


def same_values(base: torch.Tensor, tuned: torch.Tensor) -> bool:
    """Whether `tuned` is `base` up to the narrower of the two storage types (a checkpoint saved in fp16 holds the fp16 rounding of
    every tensor training left alone)."""
    if base.dtype == tuned.dtype:
        return torch.equal(base, tuned)
    return torch.equal(base.to(tuned.dtype), tuned) or torch.equal(tuned.to(base.dtype), base)


def check_states(base: dict, tuned: dict, layers: int, max_rank: int, ignore_other: bool = False):
    """Everything the two state dicts show without a launch.  Returns [(index, key)] of the targets that differ from the base."""
    if not 1 <= int(max_rank) <= 64:
        raise ValueError(f"extract_lora(): max_rank must lie in [1, 64] (got {max_rank}): the adapter bank supports rank <= 64")
    c = probe_width(max_rank)
    keys = target_keys(layers)
    wkeys = {k + ".weight" for k in keys}
    missing = sorted(k for k in wkeys if k not in tuned or k not in base)
    if missing:
        raise ValueError(f"extract_lora(): target weights missing from the checkpoint or the base: {missing[:4]}"
                         + (f" and {len(missing) - 4} more" if len(missing) > 4 else ""))
    common = [k for k in tuned if k in base and torch.is_tensor(tuned[k]) and torch.is_tensor(base[k])]
    shapes = [f"{k}: {tuple(tuned[k].shape)} against the base's {tuple(base[k].shape)}" for k in common if tuned[k].shape != base[k].shape]
    if shapes:
        raise ValueError(f"extract_lora(): shape mismatch (not a fine-tune of this base): {'; '.join(shapes[:4])}"
                         + (f" and {len(shapes) - 4} more" if len(shapes) > 4 else ""))
    for k in sorted(wkeys):
        K, N = base[k].shape
        if K % 16 or N % 16 or min(K, N) < c:
            raise ValueError(f"extract_lora(): {k} is [{K}, {N}]: both must be multiples of 16 and at least the probe width {c}")
    if not ignore_other:
        other = [k for k in common if k not in wkeys and not same_values(base[k], tuned[k])]
        if other:
            raise ValueError(f"extract_lora(): {len(other)} tensors outside the LoRA targets differ from the base (train.py freezes "
                             f"them, so this is not a LoRA of this base; ignore_other=True extracts the targets anyway): "
                             f"{other[:8]}" + (" ..." if len(other) > 8 else ""))
    return [(i, k) for i, k in enumerate(keys) if not same_values(base[k + ".weight"], tuned[k + ".weight"])]


def _orth(y: torch.Tensor) -> torch.Tensor:
    return torch.linalg.qr(y.double().cpu(), mode="reduced")[0]


def pick_rank(S: torch.Tensor):
    """(r, largest ratio) of singular values S (descending, float64): r = the index of the largest S_i / S_{i+1}, i < c - 1."""
    head, tail = S[:-1], S[1:]
    ratio = torch.where(tail > 0, head / tail.clamp_min(torch.finfo(torch.float64).tiny), torch.full_like(head, float("inf")))
    ratio = torch.where(head > 0, ratio, torch.zeros_like(ratio))
    i = int(torch.argmax(ratio))
    return i + 1, float(ratio[i])


def extract_target(project, key: str, K: int, N: int, max_rank: int, gap: float, omega: torch.Tensor):
    """One target.  project(x fp32 [rows, c] on the CPU, trans) -> D x or D^T x (any float type, any device).  Returns
    (A fp32 [r, K], B fp32 [N, r], report entry) or None for a D that is zero."""
    Q = _orth(project(omega, False))
    if not bool(torch.isfinite(Q).all()):
        raise ValueError(f"extract_lora(): {key}: the difference holds non-finite values")
    Q = _orth(project(Q.float(), True))
    Q = _orth(project(Q.float(), False))
    Q = Q.float()                                   # the Q the last product is taken with is the Q of the factorisation
    Bt = project(Q, True).double().cpu()            # [N, c]
    U, S, Vh = torch.linalg.svd(Bt.t(), full_matrices=False)
    if float(S[0]) == 0.0:
        return None
    r, ratio = pick_rank(S)
    if ratio < gap or r > max_rank:
        raise ValueError(f"extract_lora(): {key}: the difference from the base is not low-rank (largest singular-value ratio "
                         f"{ratio:.3g} at rank {r}; needs >= {gap:g} at a rank <= {max_rank}): a full fine-tune, or the wrong base")
    root = S[:r].sqrt()
    A = ((Q.double() @ U[:, :r]) * root).t().contiguous().float()
    B = (Vh[:r].t() * root).contiguous().float()
    return A, B, dict(r=r, sigma_r=float(S[r - 1]), sigma_next=float(S[r]), ratio=ratio)


def extract(base: dict, tuned: dict, layers: int, make_project, max_rank: int = 16, gap: float = 8.0, seed: int = 0,
            ignore_other: bool = False):
    """(adapters, 1.0, report).  make_project(key, base weight, tuned weight) -> the project() of extract_target for that target;
    called target by target, and only after check_states() has passed for the whole checkpoint."""
    tuned = tuned["model"] if isinstance(tuned, dict) and "model" in tuned and isinstance(tuned["model"], dict) else tuned
    changed = check_states(base, tuned, layers, max_rank, ignore_other)
    c = probe_width(max_rank)
    adapters, report = {}, {}
    for index, key in changed:
        wb, wt = base[key + ".weight"], tuned[key + ".weight"]
        K, N = wb.shape
        got = extract_target(make_project(key, wb, wt), key, K, N, int(max_rank), float(gap), draw_omega(N, c, seed, index))
        if got is not None:
            adapters[key] = (got[0], got[1])
            report[key] = got[2]
    return adapters, 1.0, report


class DeviceDelta:
    """make_project over ittv_delta_project: one upload of the target's two weights (each in its own storage type), then one launch
    per product.  One workspace serves every target."""

    def __init__(self, device):
        from indextts import _native_voice as natv
        self.natv, self.device = natv, torch.device(device)
        natv.lib()
        self.ws = natv.delta_workspace(self.device)

    @staticmethod
    def _image(w):
        w = w.detach()
        return w if w.dtype in (torch.float16, torch.bfloat16, torch.float32) else w.float()

    def __call__(self, key, wb, wt):
        wb, wt = (self._image(w).to(self.device).contiguous() for w in (wb, wt))

        def project(x, trans):
            return self.natv.delta_project(wt, wb, x.to(self.device, torch.float32).contiguous(), trans, self.ws)
        return project


def save_voice(path, adapters: dict, scaling: float):
    """One voice as a file of tensors and a float only ({'adapters': {target: {'A': .., 'B': ..}}, 'scaling': float})."""
    torch.save({"adapters": {k: {"A": A.detach().cpu().contiguous(), "B": B.detach().cpu().contiguous()} for k, (A, B) in adapters.items()},
                "scaling": float(scaling)}, path)


def load_voice(path):
    """(adapters, scaling) of a save_voice file, through the weights-only unpickler: the file cannot run code."""
    d = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(d, dict) or set(d) != {"adapters", "scaling"}:
        raise ValueError(f"{path}: not a voice file (save_voice)")
    return {k: (v["A"], v["B"]) for k, v in d["adapters"].items()}, float(d["scaling"])
