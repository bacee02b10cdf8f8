"""Tensor-level access to the native stencil kernels.

These wrap single kernels of ``csrc/kernels/stencil.hip`` for torch tensors
(device kernels on ROCm tensors, the OpenMP oracle on CPU tensors), so the
kernels can be tested against plain PyTorch fp32 and composed into custom
schedules.  Fields use the engine's memory layout (ghost ring + 256-B pitch,
``heat::Layout``); ``Field`` owns a torch tensor with that layout.

Reference kernels: ``heat`` (``cuda/cuda_heat.cu:140-163``) and the fused
``heat<threads>`` + ``semi_reduce`` residual (``:32-138``).
"""
from __future__ import annotations

import ctypes
import enum
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..models.config import INIT_MODES, check_edges, insulated_mask, periodic_mask
from ..parallel.topology import layout

Box = Tuple[int, int, int, int]  # (r0, r1, c0, c1) in local coordinates


class TbVariant(enum.IntFlag):
    """Variant flags of the temporally blocked kernel (``heat::gpu::tbv`` in
    csrc/include/heat/kernels.hpp).  The low two bits pick the register
    pipeline; the rest pick the build and the launch layout."""
    RING3 = 0             # 3-row rings, skew 1
    RING4 = 1             # 4-row rings, skew 2
    RING2 = 2             # 2-row rings + copy
    RAMP = 3              # 3-row rings + compile-time ramp skip
    SCALAR = 4            # scalar row-update build (depth 12 lives here)
    XCD_GROUPS = 16       # contiguous wave ranges per XCD
    ALT_DIRECTION = 32    # odd chunks stream bottom-up
    FLOAT2 = 64           # float2 lanes (128-column strips)
    FORCE_AGE_PAIRS = 256  # age groups even at equal weights
    DIAG_NO_STORE = 1024  # diagnostics: no output stores (wrong results)
    SPLIT = 2048          # two-wave level-split pipelines (depths 8, 12)
    DIAG_CACHED_ROWS = 4096  # diagnostics: cache-resident input rows (wrong results)
    NO_AGE_PAIRS = 16384  # never age-group
    LINEAR = 32768        # force the balanced plan: equal strip-rows per unit
    NO_LINEAR = 65536     # never switch to it (default: when the classic plan fills < 90 %)
    TILE = 131072         # workgroup tiles: 8 waves x R rows in VGPRs, LDS row exchange per step
    TILE_DPP = 262144     # with TILE: DPP lane shifts instead of ds_bpermute
    SHIFT_MIXED = 524288  # with SPLIT: west shift DPP, east ds_bpermute (tb_split_mixed.hip)
    DEFAULT = RAMP | SCALAR | XCD_GROUPS       # 23
    DEFAULT_DEEP = DEFAULT | SPLIT             # 2071


@dataclass
class TbTuning:
    """Launch-planner knobs (``heat::gpu::TbTuning``); HEAT_TB_* environment
    variables seed them when the library is first used."""
    variant: int = -1
    rounds: int = 0
    min_len: int = 0
    waves: int = 0
    edge_frac: float = 1.0
    age_weights: List[float] = field(default_factory=list)
    tile_rows: int = 0  # rows per wave of TILE launches (0: planner)
    tile_waves: int = 0  # waves per TILE workgroup, 8 or 16 (0: planner)
    tile_xl: int = -1  # TILE lane shifts: 0 DPP, 1 ds_bpermute, 2 mixed (-1: default)
    nt: int = -1  # level-split rows non-temporal 1 / plain 0 (-1: by the bytes a pass sweeps)


def tb_tuning() -> TbTuning:
    t = _native.HeatTbTuning()
    _native.call("heat_tb_get_tuning", ctypes.byref(t))
    return TbTuning(t.variant, t.rounds, t.min_len, t.waves, t.edge_frac,
                    [t.weights[i] for i in range(t.n_weights)], t.tile_rows, t.tile_waves,
                    t.tile_xl, t.nt)


def set_tb_tuning(t: TbTuning) -> None:
    n = len(t.age_weights)
    if n > 4:
        raise ValueError("at most 4 age weights")
    c = _native.HeatTbTuning(int(t.variant), int(t.rounds), int(t.min_len), int(t.waves),
                             float(t.edge_frac), n, int(t.tile_rows),
                             (ctypes.c_double * 4)(*t.age_weights), int(t.tile_waves),
                             int(t.tile_xl), int(t.nt), 0)
    _native.call("heat_tb_set_tuning", ctypes.byref(c))


@dataclass
class Geom:
    """Global placement of a local field: local (0,0) is global (gx0, gy0)."""
    nx: int
    ny: int
    gx0: int = 0
    gy0: int = 0
    cx: float = 0.1
    cy: float = 0.1


class Field:
    """A local field (owned lx x ly block + `halo`-deep ghost ring) in a torch tensor."""

    def __init__(self, lx: int, ly: int, halo: int = 1, device="cpu", fill: float = 0.0):
        self.lx, self.ly, self.halo = lx, ly, halo
        self.pitch, self.rows, self.hx, self.hy = layout(lx, ly, halo)
        self.data = torch.full((self.rows, self.pitch), fill, dtype=torch.float32,
                               device=device)

    @property
    def device(self):
        return self.data.device

    def ptr(self) -> int:
        """Address of owned cell (0, 0)."""
        return self.data.data_ptr() + 4 * (self.hx * self.pitch + self.hy)

    def view(self, r0: int, r1: int, c0: int, c1: int) -> torch.Tensor:
        """View of local cells [r0,r1) x [c0,c1) (negative = ghost ring)."""
        return self.data[self.hx + r0:self.hx + r1, self.hy + c0:self.hy + c1]

    def owned(self) -> torch.Tensor:
        return self.view(0, self.lx, 0, self.ly)

    def set_owned(self, t: torch.Tensor) -> None:
        self.owned().copy_(t)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0


def _resid_ptr(resid: Optional[torch.Tensor]) -> Optional[int]:
    if resid is None:
        return None
    if resid.dtype != torch.int32 or resid.numel() < 1:
        raise ValueError("resid must be an int32 tensor (float bits of max|delta|)")
    return resid.data_ptr()


def resid_value(resid: torch.Tensor) -> float:
    """Decode the float bits an atomic-max residual word holds."""
    return float(resid[:1].cpu().view(torch.float32).item())


def init_field(f: Field, geom: Geom, mode: str = "ref-wrap", seed: int = 0) -> None:
    """Fill every cell of the field (owned, ghosts, padding) from the initial condition."""
    m = INIT_MODES[mode]
    if f.device.type == "cpu":
        from ..models.reference import init_grid
        full = init_grid(geom.nx, geom.ny, mode, seed)  # small fields only
        f.data.zero_()
        r0, r1 = max(0, geom.gx0 - f.hx), min(geom.nx, geom.gx0 + f.lx + f.hx)
        c0, c1 = max(0, geom.gy0 - f.hy), min(geom.ny, geom.gy0 + f.pitch - f.hy)
        f.data[r0 - geom.gx0 + f.hx:r1 - geom.gx0 + f.hx, c0 - geom.gy0 + f.hy:c1 - geom.gy0 + f.hy] = \
            torch.from_numpy(full[r0:r1, c0:c1])
        return
    _native.call("heat_op_init", ctypes.c_void_p(f.ptr()), f.lx, f.ly, f.halo, geom.gx0,
                 geom.gy0, geom.nx, geom.ny, m, seed, ctypes.c_void_p(_stream()))


def naive_step(src: Field, dst: Field, geom: Geom, box: Optional[Box] = None,
               resid: Optional[torch.Tensor] = None) -> None:
    """One Jacobi step over `box` (default: the owned block)."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    if src.pitch != dst.pitch:
        raise ValueError("src/dst layouts differ")
    if src.device.type == "cpu":
        r = ctypes.c_float()
        _native.call("heat_cpu_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                     src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy,
                     r0, r1, c0, c1, ctypes.byref(r) if resid is not None else None)
        if resid is not None:
            resid.view(torch.float32)[0] = max(resid_value(resid), r.value)
        return
    rp = _resid_ptr(resid)
    _native.call("heat_op_naive_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy,
                 r0, r1, c0, c1, ctypes.c_void_p(rp) if rp else None,
                 ctypes.c_void_p(_stream()))


def lds_step(src: Field, dst: Field, geom: Geom, box: Optional[Box] = None,
             resid: Optional[torch.Tensor] = None, numerics: str = "fp32") -> None:
    """One Jacobi step over `box` with the LDS-staged tile kernel (GPU only);
    numerics "fp32" (canonical FMA) or "mpi" (reference MPI double arithmetic)."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    if src.pitch != dst.pitch:
        raise ValueError("src/dst layouts differ")
    if src.device.type != "cuda":
        raise ValueError("lds_step needs GPU fields")
    rp = _resid_ptr(resid)
    _native.call("heat_op_lds_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy,
                 r0, r1, c0, c1, ctypes.c_void_p(rp) if rp else None,
                 ctypes.c_void_p(_stream()), {"fp32": 0, "mpi": 1}[numerics])


def source_step(src: Field, dst: Field, q: Field, geom: Geom, box: Optional[Box] = None,
                resid: Optional[torch.Tensor] = None,
                gate: Optional[torch.Tensor] = None) -> None:
    """One Jacobi step over `box` with a per-cell heat source: u' = stencil(u) + q
    on every cell the step updates (one rounded fp32 add after the unchanged
    expression; fixed cells ignore q).  q has the layout of src and dst.  The
    streaming HIP kernel on GPU fields (`gate`: an int32 GPU tensor whose first
    word, if non-zero, makes the launch write nothing), its host twin on CPU
    fields.  resid: max |new - old| over the box's updated cells."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    if src.pitch != dst.pitch or src.pitch != q.pitch:
        raise ValueError("src/dst/q layouts differ")
    if src.device.type == "cpu":
        if gate is not None:
            raise ValueError("the gate is a device word: GPU fields only")
        r = ctypes.c_float()
        _native.call("heat_cpu_source_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                     ctypes.c_void_p(q.ptr()), src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny,
                     geom.cx, geom.cy, r0, r1, c0, c1,
                     ctypes.byref(r) if resid is not None else None)
        if resid is not None:
            old, new = resid[:1].clone(), torch.tensor([r.value], dtype=torch.float32)
            # The word keeps the larger of the two as unsigned float bits (a NaN on top).
            if (int(new.view(torch.int32)) & 0xFFFFFFFF) > (int(old) & 0xFFFFFFFF):
                resid[:1] = new.view(torch.int32)
        return
    rp = _resid_ptr(resid)
    if gate is not None and (gate.dtype != torch.int32 or gate.device != src.device):
        raise ValueError("gate must be an int32 tensor on the fields' device")
    _native.call("heat_op_source_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 ctypes.c_void_p(q.ptr()), src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny,
                 geom.cx, geom.cy, r0, r1, c0, c1, ctypes.c_void_p(rp) if rp else None,
                 ctypes.c_void_p(_stream()),
                 ctypes.c_void_p(gate.data_ptr()) if gate is not None else None)


def source_plan(src: Field, dst: Field, q: Field, box: Optional[Box] = None) -> dict:
    """The launch plan `source_step` takes for these GPU fields and box (strips,
    chunks, units, chunk_rows, waves, align, vector_rows) together with the
    planner's constants strip_cols, max_chunk_rows, min_chunk_rows and
    waves_per_cu."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    p = _native.HeatSourcePlan()
    _native.call("heat_op_source_plan", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 ctypes.c_void_p(q.ptr()), src.pitch, r0, r1, c0, c1, ctypes.byref(p))
    return {k: int(getattr(p, k)) for k, _ in p._fields_}


def set_source_max_waves(waves: int) -> None:
    """Cap the waves of a `source_step` launch (0: the default, 16 waves per
    CU, about half the kernel's occupancy): tests make the kernel's grid-stride
    loop run more than once with it."""
    _native.call("heat_op_source_max_waves", int(waves))


def set_source_nontemporal(mode: int) -> None:
    """For tests and tools/source_bench.py only (process-global: it changes
    every launch of every solver in the process): q loads and dst stores of
    `source_step` non-temporal (1) or plain (0); -1 = the default, non-temporal
    when a step sweeps more than 256 MiB."""
    _native.call("heat_op_source_nontemporal", int(mode))


def source_tb_step(src: Field, dst: Field, q: Field, geom: Geom, box: Optional[Box], k: int,
                   resid: Optional[torch.Tensor] = None,
                   gate: Optional[torch.Tensor] = None) -> None:
    """k fused source steps in one launch (GPU only, 2 <= k <= 8): dst on `box`
    is bit for bit what k calls of `source_step` give, call j over `box` grown
    by k-1-j on every side and clipped to the plate.  Reads src in `box` grown
    by k and q in `box` grown by k-1 (clipped to the plate), writes dst on
    `box` alone.  resid: max |u_k - u_(k-1)| over the box's updated cells."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    if src.pitch != dst.pitch or src.pitch != q.pitch:
        raise ValueError("src/dst/q layouts differ")
    if src.device.type != "cuda":
        raise ValueError("source_tb_step needs GPU fields")
    rp = _resid_ptr(resid)
    if gate is not None and (gate.dtype != torch.int32 or gate.device != src.device):
        raise ValueError("gate must be an int32 tensor on the fields' device")
    _native.call("heat_op_source_tb_step", ctypes.c_void_p(src.ptr()),
                 ctypes.c_void_p(dst.ptr()), ctypes.c_void_p(q.ptr()), src.pitch, geom.gx0,
                 geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy, r0, r1, c0, c1, int(k),
                 ctypes.c_void_p(rp) if rp else None, ctypes.c_void_p(_stream()),
                 ctypes.c_void_p(gate.data_ptr()) if gate is not None else None)


def source_tb_plan(src: Field, dst: Field, q: Field, box: Optional[Box], k: int) -> dict:
    """The launch plan `source_tb_step` takes for these fields, box and depth
    (strips, chunks, units, chunk_rows, waves, align, vector_rows, overlap,
    strip_stride) with the planner's constants.  Only the fields' addresses and
    pitch matter: with `set_source_tb_max_waves` set it needs no GPU."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    p = _native.HeatSourceTbPlan()
    _native.call("heat_source_tb_plan", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 ctypes.c_void_p(q.ptr()), src.pitch, r0, r1, c0, c1, int(k), ctypes.byref(p))
    return {name: int(getattr(p, name)) for name, _ in p._fields_ if name != "pad_"}


def set_source_tb_max_waves(waves: int) -> None:
    """Cap the waves of a `source_tb_step` launch (0: the default, 8 waves per
    CU): tests make the kernel's loop over units run more than once with it."""
    _native.call("heat_source_tb_set_max_waves", int(waves))


def source_tb_launches() -> int:
    """Fused source launches this process has enqueued so far."""
    return _native.source_tb_launches()


def mfma_step(src: Field, dst: Field, geom: Geom, box: Optional[Box] = None,
              resid: Optional[torch.Tensor] = None) -> None:
    """One Jacobi step over `box` as banded matmuls on the fp32 MFMA units
    (GPU only; rounding differs from the canonical expression by ~1 ulp)."""
    r0, r1, c0, c1 = box or (0, src.lx, 0, src.ly)
    if src.pitch != dst.pitch:
        raise ValueError("src/dst layouts differ")
    if src.device.type != "cuda":
        raise ValueError("mfma_step needs GPU fields")
    rp = _resid_ptr(resid)
    _native.call("heat_op_mfma_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy,
                 r0, r1, c0, c1, ctypes.c_void_p(rp) if rp else None,
                 ctypes.c_void_p(_stream()))


def tb_step(src: Field, dst: Field, geom: Geom, depth: int,
            boxes: Optional[Sequence[Box]] = None, resid: Optional[torch.Tensor] = None,
            waves_target: int = 0, variant: int = -1, res_level: int = 0) -> None:
    """`depth` fused Jacobi steps (temporally blocked kernel) over up to 5 boxes.

    variant: -1 = chosen per launch (TbVariant.DEFAULT, or DEFAULT_DEEP for
    large depth-12 launches); otherwise TbVariant flags.  res_level (with
    resid): the step 1..depth whose max |new - old| goes to resid (0 = the
    last; inner levels need tb_mid_residual(depth)).
    """
    if src.device.type == "cpu":
        raise ValueError("tb_step is a GPU kernel")
    if not _native.lib().heat_tb_supported(depth):
        raise ValueError(f"unsupported depth {depth}")
    if src.halo < depth or src.hy < -(-depth // 4) * 4:
        raise ValueError("ghost ring thinner than depth")
    boxes = list(boxes or [(0, src.lx, 0, src.ly)])
    arr = (ctypes.c_int64 * (4 * len(boxes)))(*[v for b in boxes for v in b])
    rp = _resid_ptr(resid)
    _native.call("heat_op_tb_step", ctypes.c_void_p(src.ptr()), ctypes.c_void_p(dst.ptr()),
                 src.pitch, geom.gx0, geom.gy0, geom.nx, geom.ny, geom.cx, geom.cy, arr,
                 len(boxes), depth, ctypes.c_void_p(rp) if rp else None,
                 ctypes.c_void_p(_stream()), waves_target, int(variant), int(res_level))


def tb_stamps(buf: Optional[torch.Tensor]) -> None:
    """Diagnostics: record per-wave clock stamps of the following tb_step
    launches into `buf` (int64 GPU tensor, 4 per wave: start, end in 100 MHz
    ticks, block, strip << 32 | chunk); None switches recording off."""
    if buf is None:
        _native.call("heat_op_tb_stamps", None, 0)
        return
    if buf.dtype != torch.int64 or buf.device.type != "cuda":
        raise ValueError("stamps need an int64 GPU tensor")
    _native.call("heat_op_tb_stamps", ctypes.c_void_p(buf.data_ptr()), buf.numel() // 4)


def pack(f: Field, box: Box, out: torch.Tensor) -> None:
    r0, r1, c0, c1 = box
    if f.device.type == "cpu":
        out.view(r1 - r0, c1 - c0).copy_(f.view(r0, r1, c0, c1))
        return
    _native.call("heat_op_pack", ctypes.c_void_p(f.ptr()), f.pitch, r0, r1, c0, c1,
                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(_stream()))


def unpack(buf: torch.Tensor, f: Field, box: Box) -> None:
    r0, r1, c0, c1 = box
    if f.device.type == "cpu":
        f.view(r0, r1, c0, c1).copy_(buf.view(r1 - r0, c1 - c0))
        return
    _native.call("heat_op_unpack", ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(f.ptr()),
                 f.pitch, r0, r1, c0, c1, ctypes.c_void_p(_stream()))


MAX_BOX_COPIES = 8  # heat::gpu::kMaxBoxCopies


def copy_boxes(f: Field, copies: Sequence[Tuple[Box, torch.Tensor]], to_buf: bool) -> None:
    """Up to MAX_BOX_COPIES boxes of `f` to (to_buf) or from their contiguous
    buffers (row-major rows x cols each) in ONE launch: the packing /
    unpacking of a whole halo exchange (heat::gpu::copy_boxes).  Empty boxes
    are skipped.  On a CPU field, the slicing of pack / unpack per box."""
    copies = list(copies)
    if f.device.type == "cpu":
        if len(copies) > MAX_BOX_COPIES:
            raise ValueError(f"copy_boxes: {len(copies)} boxes")
        for (r0, r1, c0, c1), buf in copies:
            if r1 > r0 and c1 > c0:
                (pack(f, (r0, r1, c0, c1), buf) if to_buf else unpack(buf, f, (r0, r1, c0, c1)))
        return
    n = len(copies)
    for (r0, r1, c0, c1), buf in copies:
        if buf.dtype != torch.float32 or buf.device != f.device or not buf.is_contiguous():
            raise ValueError("buffers must be contiguous float32 tensors on the field's device")
        if buf.numel() < max(0, r1 - r0) * max(0, c1 - c0):
            raise ValueError(f"buffer of {buf.numel()} floats for box {(r0, r1, c0, c1)}")
        if r1 > r0 and c1 > c0 and (r0 < -f.hx or r1 > f.rows - f.hx or c0 < -f.hy
                                    or c1 > f.pitch - f.hy):
            raise ValueError(f"box {(r0, r1, c0, c1)} outside the field's allocation")
    boxes = (ctypes.c_int64 * (4 * n))(*[v for b, _ in copies for v in b])
    bufs = (ctypes.c_void_p * n)(*[buf.data_ptr() for _, buf in copies])
    _native.call("heat_op_copy_boxes", ctypes.c_void_p(f.ptr()), f.pitch, boxes, bufs, n,
                 int(bool(to_buf)), ctypes.c_void_p(_stream()))


@dataclass
class Gate:
    """The device gate record (``heat::gpu::DeviceGate``, 8 int32 words of
    which the last three are padding)."""
    stop: int = 0        # non-zero once closed
    reason: int = 0      # 1 converged, 2 non-finite residual
    stop_check: int = 0  # ordinal of the closing check
    checks: int = 0      # checks judged while open
    last_bits: int = 0   # residual (float bits) of the last judged check

    WORDS = 8

    def tensor(self, device) -> torch.Tensor:
        w = [self.stop, self.reason, self.stop_check, self.checks, self.last_bits, 0, 0, 0]
        return torch.tensor(w, dtype=torch.int64).to(torch.int32).to(device)

    @classmethod
    def read(cls, gate: torch.Tensor) -> "Gate":
        w = [int(v) & 0xFFFFFFFF for v in gate[:5].cpu().tolist()]
        return cls(*w)


def judge(resid: torch.Tensor, gate: torch.Tensor, eps: float, mpi_compat: bool = False,
          n: int = 1, slots: int = 1, stride: int = 0) -> None:
    """The device-side convergence decision (heat::gpu::judge_check, GPU only)
    on n checks in order: check i's residual is the maximum, as unsigned
    words, of resid[s * stride + i] over s < slots; while the gate (an 8-word
    int32 tensor laid out as Gate) is open, a non-finite word closes it with
    reason 2, a word that meets eps (mpi_compat: double(r) <= eps, otherwise
    r < float32(eps)) with reason 1.  The words read are zeroed either way."""
    if resid.dtype != torch.int32 or gate.dtype != torch.int32:
        raise ValueError("resid and gate must be int32 tensors")
    if resid.device.type != "cuda" or gate.device != resid.device:
        raise ValueError("judge needs GPU tensors on one device")
    if gate.numel() < Gate.WORDS or not gate.is_contiguous() or not resid.is_contiguous():
        raise ValueError("gate must hold 8 contiguous words, resid be contiguous")
    if n >= 1 and 1 <= slots <= 64 and stride >= 0 and \
            resid.numel() < (slots - 1) * stride + n:
        raise ValueError(f"{resid.numel()} residual words for {n} checks x {slots} slots")
    _native.call("heat_op_judge", ctypes.c_void_p(resid.data_ptr()),
                 ctypes.c_void_p(gate.data_ptr()), float(eps), int(bool(mpi_compat)), int(n),
                 int(slots), int(stride), ctypes.c_void_p(_stream()))


def checksum(f: Field, ox: int = 0, oy: int = 0, ny: Optional[int] = None) -> dict:
    """Checksum of the field's owned block placed at (ox, oy) of a plate with
    `ny` columns (default: the block's own): {"hash": wrapping u64 sum of
    mix64(global index * 0x100000001B3 ^ bits) as an int, "sum" (float64),
    "min", "max", "count"}.  The device kernel on a GPU field (its sum follows
    no fixed order), the host heat::checksum_block on a CPU field.  Hashes and
    counts of disjoint blocks add up to the plate's."""
    ny = f.ly if ny is None else int(ny)
    c = _native.HeatChecksum()
    if f.device.type == "cpu":
        _native.call("heat_cpu_checksum", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly, int(ox),
                     int(oy), ny, ctypes.byref(c))
    else:
        _native.call("heat_op_checksum", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly, int(ox),
                     int(oy), ny, ctypes.byref(c), ctypes.c_void_p(_stream()))
    return {"hash": int(c.hash), "sum": c.sum, "min": c.min, "max": c.max, "count": int(c.count)}


def coarse_dims(nx: int, ny: int, fx: int, fy: int) -> Tuple[int, int]:
    """Rows and columns (ceil(nx / fx), ceil(ny / fy)) of the coarse view of an
    nx x ny plate; raises on a factor < 1 or above the limit of 2**22 cells."""
    cr, cc = ctypes.c_int64(0), ctypes.c_int64(0)
    _native.call("heat_coarse_dims", int(nx), int(ny), int(fx), int(fy), ctypes.byref(cr),
                 ctypes.byref(cc))
    return int(cr.value), int(cc.value)


def coarse(f: Field, fx: int, fy: int, ox: int = 0, oy: int = 0, nx: Optional[int] = None,
           ny: Optional[int] = None, out: Optional[dict] = None) -> dict:
    """Coarse view of the field's owned block placed at (ox, oy) of an nx x ny
    plate (default: the block is the plate): coarse cell (I, J) covers plate
    rows [I*fx, (I+1)*fx) and columns [J*fy, (J+1)*fy), cut at the plate's edge.
    Returns {"sum": float64, "min", "max": float32} tensors of shape
    (ceil(nx/fx), ceil(ny/fy)) on the field's device and "count" (int64, the
    geometric cell counts).  A cell that holds a NaN is NaN in all three.
    `out`: the dict of an earlier call, into which this (disjoint) block is
    merged.  The device kernel on a GPU field (enqueued on the current stream),
    the host heat::coarse_block on a CPU field."""
    nx = f.lx if nx is None else int(nx)
    ny = f.ly if ny is None else int(ny)
    fx, fy = int(fx), int(fy)
    cr, cc = coarse_dims(nx, ny, fx, fy)
    if out is None:
        dev = f.device
        out = {"sum": torch.zeros((cr, cc), dtype=torch.float64, device=dev),
               "min": torch.full((cr, cc), float("inf"), dtype=torch.float32, device=dev),
               "max": torch.full((cr, cc), float("-inf"), dtype=torch.float32, device=dev)}
    for k, dt in (("sum", torch.float64), ("min", torch.float32), ("max", torch.float32)):
        t = out[k]
        if (t.dtype != dt or tuple(t.shape) != (cr, cc) or not t.is_contiguous()
                or t.device != f.device):
            raise ValueError(f"out[{k!r}] must be a contiguous {dt} ({cr}, {cc}) tensor on "
                             f"{f.device}")
    args = (ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly, int(ox), int(oy), nx, ny, fx, fy,
            ctypes.c_void_p(out["sum"].data_ptr()), ctypes.c_void_p(out["min"].data_ptr()),
            ctypes.c_void_p(out["max"].data_ptr()))
    if f.device.type == "cpu":
        _native.call("heat_cpu_coarse", *args)
    else:
        _native.call("heat_op_coarse", *args, ctypes.c_void_p(_stream()))
    rows = torch.clamp(torch.arange(1, cr + 1, dtype=torch.int64) * fx, max=nx) - \
        torch.arange(cr, dtype=torch.int64) * fx
    cols = torch.clamp(torch.arange(1, cc + 1, dtype=torch.int64) * fy, max=ny) - \
        torch.arange(cc, dtype=torch.int64) * fy
    out["count"] = rows[:, None] * cols[None, :]
    return out


def coarse_plan(f: Field, fx: int, fy: int, ox: int = 0, oy: int = 0) -> dict:
    """The launch plan `coarse` takes for this GPU field (strips, chunks, units,
    waves, ...) together with the planner's constants strip_cols,
    max_chunk_rows, min_chunk_rows and waves_per_cu."""
    p = _native.HeatCoarsePlan()
    _native.call("heat_op_coarse_plan", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly, int(ox),
                 int(oy), int(fx), int(fy), ctypes.byref(p))
    return {k: int(getattr(p, k)) for k, _ in p._fields_ if k != "pad_"}


def set_coarse_max_waves(waves: int) -> None:
    """Cap the waves of a `coarse` launch (0: the default, from the CU count):
    tests make the kernel's grid-stride loop run more than once with it."""
    _native.call("heat_op_coarse_max_waves", int(waves))


def _wrap_mask(wrap: str) -> int:
    if any(c not in "xy" for c in wrap):
        raise ValueError(f"wrap={wrap!r}; expected any of the letters 'xy'")
    return (1 if "x" in wrap else 0) | (2 if "y" in wrap else 0)


def refine_axis(n: int, f: int, order: int = 1, wrap: bool = False):
    """The engine's refinement table of an axis of n cells refined by f
    (heat::refine_axis): NumPy arrays i0, i1 (int32) and w (float32)."""
    n = int(n)
    i0 = np.empty(max(n, 0), np.int32)
    i1 = np.empty(max(n, 0), np.int32)
    w = np.empty(max(n, 0), np.float32)
    _native.call("heat_refine_axis", n, int(f), int(order), int(bool(wrap)),
                 ctypes.c_void_p(i0.ctypes.data), ctypes.c_void_p(i1.ctypes.data),
                 ctypes.c_void_p(w.ctypes.data))
    return i0, i1, w


def refine(f: Field, S, fx: int, fy: int, order: int = 1, wrap: str = "", ox: int = 0,
           oy: int = 0, nx: Optional[int] = None, ny: Optional[int] = None) -> None:
    """Fill the field's owned block, placed at (ox, oy) of an nx x ny plate
    (default: the block is the plate), from the (ceil(nx/fx), ceil(ny/fy))
    source grid S by refinement: piecewise constant (order 0) or cell-centred
    bilinear (order 1), the axes in `wrap` (letters of "xy") wrapping, the
    others clamping (reference.refine_np is the definition).  Writes owned
    cells only.  The device kernel on a GPU field (enqueued on the current
    stream and waited for), the host heat::refine_block on a CPU field."""
    nx = f.lx if nx is None else int(nx)
    ny = f.ly if ny is None else int(ny)
    if not isinstance(S, torch.Tensor):
        S = torch.from_numpy(np.array(S, dtype=np.float32))  # a copy: S may be read-only
    S = S.to(device=f.device, dtype=torch.float32).contiguous()
    if S.dim() != 2:
        raise ValueError(f"source grid shape {tuple(S.shape)}: expected (rows, cols)")
    args = (ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly, int(ox), int(oy), nx, ny,
            ctypes.c_void_p(S.data_ptr()), int(S.shape[0]), int(S.shape[1]), int(fx), int(fy),
            int(order), _wrap_mask(wrap))
    if f.device.type == "cpu":
        _native.call("heat_cpu_refine", *args)
    else:
        _native.call("heat_op_refine", *args, ctypes.c_void_p(_stream()))


def refine_plan(f: Field) -> dict:
    """The launch plan `refine` takes for this GPU field (strips, chunks, units,
    chunk_rows, waves, align, vector_rows) together with the planner's constants
    strip_cols, max_chunk_rows, min_chunk_rows and waves_per_cu."""
    p = _native.HeatRefinePlan()
    _native.call("heat_op_refine_plan", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly,
                 ctypes.byref(p))
    return {k: int(getattr(p, k)) for k, _ in p._fields_}


def set_refine_max_waves(waves: int) -> None:
    """Cap the waves of a `refine` launch (0: the default, from the CU count):
    tests make the kernel's grid-stride loop run more than once with it."""
    _native.call("heat_op_refine_max_waves", int(waves))


def fill_insulated_ghosts(f: Field, sides: str, depth: int) -> None:
    """Insulated (zero-flux) plate edges: fill the field's ghost frame, `depth`
    cells deep, beyond every side in `sides` (letters of "nswe", or "all")
    with the field's mirror image across that edge row / column (the edge cell
    not repeated, both reflections beyond two insulated sides).  Only cells
    beyond at least one of those sides are written.  One HIP launch on a GPU
    field; the host twin the CPU backend uses on a CPU field."""
    mask = insulated_mask(sides)
    if depth < 1 or depth > f.halo:
        raise ValueError(f"depth {depth} outside the field's ghost ring ({f.halo})")
    if (mask & 3 and f.lx <= depth) or (mask & 12 and f.ly <= depth):
        raise ValueError(f"a {f.lx} x {f.ly} field cannot mirror {depth} rows/columns")
    if f.device.type == "cpu":
        _native.call("heat_cpu_fill_insulated_ghosts", ctypes.c_void_p(f.ptr()), f.pitch, f.lx,
                     f.ly, mask, depth)
        return
    _native.call("heat_op_fill_insulated_ghosts", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly,
                 mask, depth, ctypes.c_void_p(_stream()))


def fill_edge_ghosts(f: Field, insulated: str, periodic: str, depth: int) -> None:
    """The general fill of the field's ghost frame, `depth` cells deep: the
    mirror image beyond every side in `insulated` (as fill_insulated_ghosts),
    the field's opposite edge beyond both sides of every axis in `periodic`
    (letters of "xy": (r < 0, c) := (r + lx, c), (r >= lx, c) := (r - lx, c),
    likewise for columns), composed per axis in the corners.  An axis cannot be
    wrapped and mirrored; a wrapped axis needs an extent >= depth.  One HIP
    launch on a GPU field; the host twin the CPU backend uses on a CPU field."""
    check_edges(insulated, periodic)
    ins, per = insulated_mask(insulated), periodic_mask(periodic)
    if depth < 1 or depth > f.halo:
        raise ValueError(f"depth {depth} outside the field's ghost ring ({f.halo})")
    if (ins & 3 and f.lx <= depth) or (ins & 12 and f.ly <= depth):
        raise ValueError(f"a {f.lx} x {f.ly} field cannot mirror {depth} rows/columns")
    if (per & 1 and f.lx < depth) or (per & 2 and f.ly < depth):
        raise ValueError(f"a {f.lx} x {f.ly} field cannot wrap {depth} rows/columns")
    if f.device.type == "cpu":
        _native.call("heat_cpu_fill_edge_ghosts", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly,
                     ins, per, depth)
        return
    _native.call("heat_op_fill_edge_ghosts", ctypes.c_void_p(f.ptr()), f.pitch, f.lx, f.ly,
                 ins, per, depth, ctypes.c_void_p(_stream()))


def residual(a: Field, b: Field, box: Optional[Box] = None,
             resid: Optional[torch.Tensor] = None) -> float:
    """max |a - b| over `box` (owned block by default)."""
    r0, r1, c0, c1 = box or (0, a.lx, 0, a.ly)
    if a.device.type == "cpu":
        return float((a.view(r0, r1, c0, c1) - b.view(r0, r1, c0, c1)).abs().max())
    own = resid is None
    if own:
        resid = torch.zeros(1, dtype=torch.int32, device=a.device)
    _native.call("heat_op_residual", ctypes.c_void_p(a.ptr()), ctypes.c_void_p(b.ptr()),
                 a.pitch, r0, r1, c0, c1, ctypes.c_void_p(resid.data_ptr()),
                 ctypes.c_void_p(_stream()))
    return resid_value(resid) if own else float("nan")
