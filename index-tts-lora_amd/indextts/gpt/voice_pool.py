"""Voice pool: any number of LoRA voices paged through the slots of the adapter bank.

The bank of GPTEngine.attach_lora_bank multiplies [x | u] by [W ; B_bank^T]: a row's shrink vector u is zero in every slot the
row does not name, and itts_lora_shrink rewrites all Kx columns of u on every call.  So the n slots of the bank can be a CACHE
over a pool of any size: which voice sits in a slot is data, the captured step never notices.

Image layout.  The packed weight (include/indextts_hip.h, "Packed weight layout") stores W[K][N] as 1-KiB blocks block(nt, ks),
nt = n / 16, ks = k / KS, KS = 32 (bf16 / f16) or 16 (f32), in the order nt * KT + ks (ks innermost).  Inside a block lane
l = (g << 4) | c owns the 16 contiguous bytes W[ks * KS + g * E + e][nt * 16 + c], e = 0..E-1, E = 8 or 4.  Hence
  * 16-bit: rows ks * 32 + 0..15 of a column tile are lanes g = 0, 1 = bytes [0, 512) of the block, rows 16..31 bytes [512, 1024);
  * f32:    rows ks * 16 + 0..15 are the whole block;
either way a unit of 16 consecutive k rows (16-aligned) is 16 * 16 * sizeof(T) contiguous bytes, and consecutive units are
consecutive in memory within one column tile (two per block, then the next ks).  The extended weight [W ; B_bank^T] has
K % KS == 0 base rows, so slot a of padded rank rp -- rows K + a * rp ... + rp -- is, for each of the NT = N / 16 column tiles,
ONE contiguous run of rp * 16 * sizeof(T) bytes at byte
      nt * KT * 1024 + (K / KS) * 1024 + a * rp * 16 * sizeof(T),         KT = (K + Kx) / KS,
of the extended weight (span()).  A voice's B-image is [NT][that run]: nat.pack_weight of its zero-padded B^T [rp, N] (the
packer pads K to whole k-steps with zeros behind the run), the same rounding and the same bits as the bank's re-pack.  Its
A-image is T [rp][K] = T(A * scaling), the scaling folded in at fp32 before the rounding: what attach_lora_bank puts into bank_a_*.

Cost per voice and layer: rp * (sum K + sum N) * sizeof(T) over the targets -- 15.7 MB at 24 layers, rp = 16, bf16, four targets.

Residency and admit_voices are host code only (no device, no torch).
"""
from __future__ import annotations

import weakref

TARGETS = (("attn.c_attn", "w_qkv"), ("attn.c_proj", "w_o"), ("mlp.c_fc", "w_fc"), ("mlp.c_proj", "w_pr"))   # GPTEngine.BANK_TARGETS


def target_shape(wkey: str, D: int):
    """(K, N) of a block's GEMM at model width D."""
    return {"w_qkv": (D, 3 * D), "w_o": (D, D), "w_fc": (D, 4 * D), "w_pr": (4 * D, D)}[wkey]


def span(K: int, N: int, Kx: int, slot: int, rp: int, itemsize: int):
    """Where slot `slot` of padded rank rp lies in the packed [K + Kx][N] weight of elements of `itemsize` bytes:
    (NT, tile stride, offset, run) -- for nt in [0, NT) the bytes [nt * stride + offset, + run)."""
    KS = 16 if itemsize == 4 else 32
    if K % KS or Kx % KS or N % 16 or rp % 16 or slot < 0 or (slot + 1) * rp > Kx:
        raise ValueError(f"span(): K={K}, N={N}, Kx={Kx}, slot={slot}, rp={rp} is no slot of a packed bank weight")
    run = rp * 16 * itemsize
    return N // 16, (K + Kx) // KS * 1024, K // KS * 1024 + slot * run, run


class Residency:
    """Which voice sits in which of `slots` bank slots: voice -> slot and back, a pin count per voice, an LRU clock.  Eviction
    is bookkeeping only: a stale slot is harmless because every row's u is zero there."""

    def __init__(self, slots: int):
        slots = int(slots)
        if slots < 1:
            raise ValueError("Residency: at least one slot")
        self.slots = slots
        self.slot_of = {}                       # voice -> slot
        self.voice_in = [None] * slots          # slot -> voice | None
        self.pins = {}                          # voice -> count (> 0)
        self.guards = {}                        # voice -> count (> 0): named by an item that waits; not to be removed, free to be evicted
        self.used = [0] * slots                 # slot -> clock of its last acquire
        self.clock = 0
        self.loads = self.hits = self.evictions = 0

    def resident(self):
        return list(self.voice_in)

    def pinned(self, voice) -> bool:
        return self.pins.get(voice, 0) > 0

    def pin(self, voices):
        for v in voices:
            self.pins[v] = self.pins.get(v, 0) + 1

    def unpin(self, voices):
        for v in voices:
            c = self.pins.get(v, 0)
            if c < 1:
                raise ValueError(f"Residency.unpin(): voice {v} holds no pin")
            if c == 1:
                del self.pins[v]
            else:
                self.pins[v] = c - 1

    def guard(self, voices):
        for v in voices:
            self.guards[v] = self.guards.get(v, 0) + 1

    def unguard(self, voices):
        for v in voices:
            if self.guards.get(v, 0) <= 1:
                self.guards.pop(v, None)
            else:
                self.guards[v] -= 1

    def held(self, voice) -> bool:
        """Pinned or guarded: the pool must keep this voice."""
        return self.pinned(voice) or voice in self.guards

    def acquire(self, voices):
        """Make every voice of `voices` resident at once.  Residents keep their slot; misses take empty slots first, then the
        least recently used unpinned slot.  Returns [(slot, voice)] to load.  ValueError -- before anything changes -- when the
        distinct voices exceed the slots, or what is empty plus unpinned."""
        want = list(dict.fromkeys(voices))
        if len(want) > self.slots:
            raise ValueError(f"{len(want)} distinct voices named at once, the bank has {self.slots} slots")
        miss = [v for v in want if v not in self.slot_of]
        keep = set(want)
        empty = [s for s in range(self.slots) if self.voice_in[s] is None]
        lru = sorted((s for s in range(self.slots) if self.voice_in[s] is not None and self.voice_in[s] not in keep
                      and not self.pinned(self.voice_in[s])), key=lambda s: self.used[s])
        if len(miss) > len(empty) + len(lru):
            raise ValueError(f"{len(miss)} voices to page in, but only {len(empty)} slots are empty and {len(lru)} unpinned "
                             f"(of {self.slots})")
        self.clock += 1
        self.hits += len(want) - len(miss)
        loads = []
        for v, s in zip(miss, empty + lru):
            old = self.voice_in[s]
            if old is not None:
                del self.slot_of[old]
                self.evictions += 1
            self.voice_in[s], self.slot_of[v] = v, s
            loads.append((s, v))
        self.loads += len(loads)
        for v in want:
            self.used[self.slot_of[v]] = self.clock
        return loads

    def drop(self, voice):
        """The voice has left its pool: its slot is empty again.  ValueError while it is pinned."""
        if self.held(voice):
            raise ValueError(f"voice {voice} is pinned or awaited by a queued item: it cannot be removed now")
        s = self.slot_of.pop(voice, None)
        if s is not None:
            self.voice_in[s] = None

    def copy_unpinned(self) -> "Residency":
        """The same arrangement with no pins (a fork's own bookkeeping over its own copy of the bank)."""
        r = Residency(self.slots)
        r.slot_of, r.voice_in, r.used, r.clock = dict(self.slot_of), list(self.voice_in), list(self.used), self.clock
        return r


def admit_voices(res: Residency, item_voices) -> int:
    """Voice-aware admission of fed items (GPTEngine.decode_refill), host only: item j names the voices item_voices[j] and, once
    placed, pins them.  Items are admitted in order while the pinned voices plus theirs fit the slots; the first that does not
    -- and every later one -- waits.  Returns the number admitted.  With nothing pinned an item alone always fits (a mix is
    refused at check time when it is wider than the slots)."""
    held = set(res.pins)
    for j, vs in enumerate(item_voices):
        if len(held | set(vs)) > res.slots:
            return j
        held |= set(vs)
    return len(item_voices)


def mix_voices(mix):
    """The voice ids a normalised mix ((id, weight), ...) names."""
    return [i for i, _ in mix]


class VoicePool:
    """Device images of any number of voices, ready to be copied into a bank slot (module docstring).  engine_shape: (layers,
    model_dim), or an engine.  rp: the padded rank of a slot (a multiple of 16, at most 64).  targets: (layer, weight key) pairs,
    default all four on every layer.  Voice ids count up from 0 and are never reused; capacity grows by doubling."""

    def __init__(self, engine_shape, rp: int, targets=None, dtype=None, device="cuda"):
        import torch
        if hasattr(engine_shape, "L"):
            dtype = engine_shape.dtype if dtype is None else dtype
            device = engine_shape.device
            engine_shape = (engine_shape.L, engine_shape.D)
        self.L, self.D = (int(v) for v in engine_shape)
        self.rp = int(rp)
        if self.rp < 16 or self.rp % 16 or self.rp > 64:
            raise ValueError(f"VoicePool: rp must be 16, 32, 48 or 64 (got {rp})")
        self.dtype = torch.bfloat16 if dtype is None else dtype
        self.device = torch.device(device)
        if targets is None:
            targets = [(i, wkey) for i in range(self.L) for _, wkey in TARGETS]
        self.targets = tuple((int(i), str(k)) for i, k in targets)
        names = {wkey: name for name, wkey in TARGETS}
        if not self.targets or any(k not in names or not 0 <= i < self.L for i, k in self.targets):
            raise ValueError(f"VoicePool: targets are (layer in [0, {self.L}), one of {sorted(names)})")
        self._key = {f"gpt.h.{i}.{names[k]}": (i, k) for i, k in self.targets}
        self._cap = 0
        self._a, self._b = {}, {}               # (layer, wkey) -> T [cap, rp, K] | uint8 [cap, NT, run]
        self._row = {}                          # live voice id -> storage row
        self._free_rows = []
        self._next = 0
        self._residencies = weakref.WeakSet()   # of the engines this pool is attached to (remove() asks them)

    def __len__(self):
        return len(self._row)

    def alive(self, voice) -> bool:
        return voice in self._row

    def nbytes_per_voice(self) -> int:
        import torch
        es = torch.empty(0, dtype=self.dtype).element_size()
        return sum(self.rp * sum(target_shape(k, self.D)) * es for _, k in self.targets)

    def _grow(self):
        import torch
        cap = max(1, 2 * self._cap)
        es = torch.empty(0, dtype=self.dtype).element_size()
        for t in self.targets:
            K, N = target_shape(t[1], self.D)
            a = torch.zeros(cap, self.rp, K, dtype=self.dtype, device=self.device)
            b = torch.zeros(cap, N // 16, self.rp * 16 * es, dtype=torch.uint8, device=self.device)
            if self._cap:
                a[: self._cap], b[: self._cap] = self._a[t], self._b[t]
            self._a[t], self._b[t] = a, b
        self._free_rows.extend(range(cap - 1, self._cap - 1, -1))
        self._cap = cap

    def add(self, adapters: dict, scaling: float) -> int:
        """One voice in the attach_lora format: {"gpt.h.{i}.attn.c_proj": (A [r, K], B [N, r]), ...}; a target it does not name
        gets a zero image.  ValueError (nothing is stored): a rank above rp, an unknown target, wrong shapes."""
        import torch
        from .. import _native as nat
        adapters, sc = dict(adapters), float(scaling)
        bad = sorted(set(adapters) - set(self._key))
        if bad:
            raise ValueError(f"VoicePool.add(): unknown adapter targets {bad}")
        for key, (A, Bm) in adapters.items():
            K, N = target_shape(self._key[key][1], self.D)
            r = int(A.shape[0])
            if r > self.rp:
                raise ValueError(f"VoicePool.add(): {key} has rank {r}, the pool's slots hold rank {self.rp}")
            if tuple(A.shape) != (r, K) or tuple(Bm.shape) != (N, r):
                raise ValueError(f"VoicePool.add(): {key}: A must be [r, {K}] and B [{N}, r]")
        if not self._free_rows:
            self._grow()
        row = self._free_rows.pop()
        dev, T = self.device, self.dtype
        for key, t in self._key.items():
            if key not in adapters:
                self._a[t][row].zero_()
                self._b[t][row].zero_()
                continue
            K, N = target_shape(t[1], self.D)
            A, Bm = (x.detach().to(dev, torch.float32) for x in adapters[key])
            r = A.shape[0]
            a = torch.zeros(self.rp, K, dtype=torch.float32, device=dev)
            a[:r] = A * sc                                                    # the scaling rides on A, folded in at fp32
            bt = torch.zeros(self.rp, N, dtype=torch.float32, device=dev)
            bt[:r] = Bm.t()
            self._a[t][row] = a.to(T)
            run = self._b[t].shape[2]
            self._b[t][row] = nat.pack_weight(bt.to(T).contiguous()).view(N // 16, -1)[:, :run]
        vid, self._next = self._next, self._next + 1
        self._row[vid] = row
        return vid

    def remove(self, voice: int):
        """The voice leaves the pool; its id is never reused and naming it later is a ValueError.  A resident voice frees its slot;
        ValueError while an engine holds a pin on it."""
        if voice not in self._row:
            raise ValueError(f"VoicePool.remove(): no voice {voice} in the pool")
        res = list(self._residencies)
        for r in res:
            if r.held(voice):
                raise ValueError(f"VoicePool.remove(): voice {voice} is pinned by an engine (a batch, a queued row or an item that "
                                 "waits for a slot speaks with it)")
        for r in res:
            r.drop(voice)
        self._free_rows.append(self._row.pop(voice))

    def images(self, voice: int, target):
        """(A-image T [rp, K], B-image uint8 [NT, run]) of a live voice: views of the pool's storage."""
        row = self._row[voice]
        return self._a[target][row], self._b[target][row]
