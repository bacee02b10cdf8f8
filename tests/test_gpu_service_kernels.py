"""The small kernels around the stencil, each on its own through its op
binding: checksum_kernel against the NumPy oracle and the host twin,
box_copy_kernel (every halo pack / unpack) against NumPy slicing,
judge_kernel (every device-judged convergence decision) against a plain
Python statement of its contract in kernels.hpp, and the stand-alone residual.
Every case is one or a few launches on small fields.  Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

from parallel_heat_amd import _native, ops

from . import service_cases as SC

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


# ---------------------------------------------------------------------------
# checksum
# ---------------------------------------------------------------------------
# (5000, 3): more rows than the 2048 / gx grid rows, the row stride loops;
# (3, 9000): more columns than 16 * 256 threads, the column stride loops.
@pytest.mark.parametrize("name", SC.CHECKSUM_SETS)
@pytest.mark.parametrize("lx,ly", SC.CHECKSUM_SHAPES + [(5000, 3), (3, 9000)])
def test_checksum_device_vs_oracle_and_host(gpu, lx, ly, name):
    v = SC.checksum_values(name, lx, ly)
    got = ops.checksum(SC.field_of(v, gpu))
    SC.assert_checksum(got, v, what=f"device {name} {lx}x{ly}")
    host = ops.checksum(SC.field_of(v, CPU))
    for key in ("hash", "count", "min", "max"):
        assert got[key] == host[key], key


@pytest.mark.parametrize("px,py", [(2, 2), (3, 1)])
def test_checksum_blocks_add_up(gpu, px, py):
    SC.check_decomposition(gpu, px, py)


def test_checksum_large_indices(gpu):
    SC.check_large_indices(gpu)


def test_checksum_sensitivity(gpu):
    SC.check_sensitivity(gpu)


def test_checksum_nan(gpu):
    SC.check_nan(gpu)


# ---------------------------------------------------------------------------
# box copies
# ---------------------------------------------------------------------------
GUARD = np.int32(0x5A5A5A5A)


def _payload_field(lx, ly, halo, device, rng, first=0):
    """Every cell (owned, ghost, padding) a NaN with its own payload, except an
    owned block of random values with -0.0 and subnormals in it."""
    f = ops.Field(lx, ly, halo, device)
    a = SC.payload_array(f, first)
    own = (rng.random((lx, ly), np.float32) * 200 - 100).astype(np.float32)
    flat = own.ravel()
    flat[::7] = -0.0
    flat[3::11] = np.float32(1e-41)    # subnormal
    flat[5::13] = np.float32(-3e-45)   # the smallest subnormals
    a[f.hx:f.hx + lx, f.hy:f.hy + ly] = own
    f.data.copy_(torch.from_numpy(a))
    return f, a


def _guarded(n, device):
    """A buffer of n floats (as int32 bits, all guard words) + 2 guard words."""
    return torch.full((n + 2,), int(GUARD), dtype=torch.int32, device=device)


def _as_f32(t):
    return t.view(torch.float32)


def _cut(a, f, b):
    return a[f.hx + b[0]:f.hx + b[1], f.hy + b[2]:f.hy + b[3]]


def _i32(x):
    return np.ascontiguousarray(x).view(np.int32)


def _check_buffers(bufs, boxes, a, f):
    for buf, b in zip(bufs, boxes):
        got = buf.cpu().numpy()
        n = SC.box_size(b)
        assert np.array_equal(got[:n], _i32(_cut(a, f, b)).ravel()), b
        assert (got[n:] == GUARD).all(), ("guard words", b)


@pytest.mark.parametrize("lx,ly", [(13, 17), (33, 70), (300, 130)])
@pytest.mark.parametrize("k", [1, 3, 8, 12])
def test_copy_boxes_exchange(gpu, k, lx, ly):
    rng = np.random.default_rng(k * 1000 + lx)
    src, a = _payload_field(lx, ly, k, gpu, rng)
    dst, b = _payload_field(lx, ly, k, gpu, rng, first=a.size)
    pairs = SC.exchange_boxes(lx, ly, k)
    sends, recvs = [p[0] for p in pairs], [p[1] for p in pairs]
    bufs = [_guarded(SC.box_size(s), gpu) for s in sends]
    ops.copy_boxes(src, [(s, _as_f32(buf)) for s, buf in zip(sends, bufs)], True)
    ops.copy_boxes(dst, [(r, _as_f32(buf)) for r, buf in zip(recvs, bufs)], False)
    torch.cuda.synchronize()
    _check_buffers(bufs, sends, a, src)
    want = b.copy()
    for s, r in pairs:
        _cut(want, dst, r)[...] = _cut(a, src, s)
    # ghost boxes = source boxes, every other cell of the target unchanged
    assert np.array_equal(_i32(dst.data.cpu().numpy()), _i32(want))
    assert np.array_equal(_i32(src.data.cpu().numpy()), _i32(a))
    # ... and box by box what the single-box kernels give
    third = ops.Field(lx, ly, k, gpu)
    third.data.copy_(torch.from_numpy(b))
    for (s, r), buf in zip(pairs, bufs):
        one = _guarded(SC.box_size(s), gpu)
        ops.pack(src, s, _as_f32(one))
        ops.unpack(_as_f32(one), third, r)
        assert torch.equal(one, buf), s
    torch.cuda.synchronize()
    assert torch.equal(third.data.view(torch.int32), dst.data.view(torch.int32))


def test_copy_boxes_strides(gpu):
    # 2600 x 2: more rows than the 2048 blocks of the grid (the row stride
    # loops); 3 x 300: more columns than the 128 threads (the column stride
    # loops), and blocks beyond its 3 rows idle.  One launch.
    rng = np.random.default_rng(5)
    src, a = _payload_field(2600, 300, 1, gpu, rng)
    dst, b = _payload_field(2600, 300, 1, gpu, rng, first=a.size)
    boxes = [(0, 2600, 297, 299), (1, 4, 0, 300)]
    targets = [(0, 2600, 299, 301), (2596, 2599, -1, 299)]  # disjoint, into ghost columns
    bufs = [_guarded(SC.box_size(x), gpu) for x in boxes]
    ops.copy_boxes(src, [(x, _as_f32(buf)) for x, buf in zip(boxes, bufs)], True)
    ops.copy_boxes(dst, [(t, _as_f32(buf)) for t, buf in zip(targets, bufs)], False)
    torch.cuda.synchronize()
    _check_buffers(bufs, boxes, a, src)
    want = b.copy()
    for s, t in zip(boxes, targets):
        _cut(want, dst, t)[...] = _cut(a, src, s)
    assert np.array_equal(_i32(dst.data.cpu().numpy()), _i32(want))
    assert np.array_equal(_i32(src.data.cpu().numpy()), _i32(a))


def test_copy_boxes_list_handling(gpu):
    rng = np.random.default_rng(6)
    lx, ly = 33, 70
    src, a = _payload_field(lx, ly, 3, gpu, rng)
    # kMaxBoxCopies boxes, all different in shape and place
    full = [(0, 33, 0, 3), (0, 33, 67, 70), (-3, 0, -3, 0), (33, 36, 70, 73), (5, 6, 0, 70),
            (0, 1, 10, 11), (10, 20, 30, 45), (-3, 36, -3, -2)]
    assert len(full) == ops.MAX_BOX_COPIES
    bufs = [_guarded(SC.box_size(x), gpu) for x in full]
    ops.copy_boxes(src, [(x, _as_f32(buf)) for x, buf in zip(full, bufs)], True)
    torch.cuda.synchronize()
    _check_buffers(bufs, full, a, src)
    # Empty boxes at positions 0, 3 and 7: the launch compacts the list, and
    # every remaining buffer must stay with its own box.
    boxes = list(full)
    boxes[0], boxes[3], boxes[7] = (4, 4, 0, 70), (0, 33, 9, 9), (20, 10, 0, 5)
    bufs = [_guarded(SC.box_size(x), gpu) for x in boxes]
    ops.copy_boxes(src, [(x, _as_f32(buf)) for x, buf in zip(boxes, bufs)], True)
    torch.cuda.synchronize()
    _check_buffers(bufs, boxes, a, src)
    # ... on the way back too
    dst, b = _payload_field(lx, ly, 3, gpu, rng, first=a.size)
    ops.copy_boxes(dst, [(x, _as_f32(buf)) for x, buf in zip(boxes, bufs)], False)
    torch.cuda.synchronize()
    want = b.copy()
    for x in boxes:
        if SC.box_size(x):
            _cut(want, dst, x)[...] = _cut(a, src, x)
    assert np.array_equal(_i32(dst.data.cpu().numpy()), _i32(want))
    # n = 0 and a list of empty boxes launch nothing
    ops.copy_boxes(dst, [], False)
    ops.copy_boxes(dst, [((2, 2, 0, 5), _as_f32(_guarded(0, gpu)))], False)
    torch.cuda.synchronize()
    assert np.array_equal(_i32(dst.data.cpu().numpy()), _i32(want))
    with pytest.raises(_native.NativeError, match="9 boxes"):
        ops.copy_boxes(src, [((0, 1, 0, 1), _as_f32(_guarded(1, gpu)))] * 9, True)
    torch.cuda.synchronize()
    assert np.array_equal(_i32(src.data.cpu().numpy()), _i32(a))


# ---------------------------------------------------------------------------
# judge
# ---------------------------------------------------------------------------
PAD = [0x11111111, 0x22222222, 0x33333333]  # the record's padding words
RGUARD = 0x0BADBEEF                          # words the kernel must not touch
FRONT = 4                                    # guard words before the list


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def judge_oracle(words, gate, eps, mpi, n, slots, stride):
    """kernels.hpp's contract of judge_check on a list of unsigned words and a
    gate [stop, reason, stop_check, checks, last_bits, pad x 3]."""
    words, gate = list(words), list(gate)
    for i in range(n):
        v = max(words[s * stride + i] for s in range(slots))  # as unsigned
        if gate[0] != 0:
            continue  # judged only while the gate is open
        ordinal = gate[3]
        gate[3] = ordinal + 1
        gate[4] = v
        if v & 0x7F800000 == 0x7F800000:
            why = 2
        else:
            r = np.uint32(v).view(np.float32)
            why = 1 if (float(r) <= float(eps) if mpi else r < np.float32(eps)) else 0
        if why:
            gate[0], gate[1], gate[2] = 1, why, ordinal
    for s in range(slots):
        for i in range(n):
            words[s * stride + i] = 0  # open or not
    return words, gate


def run_judge(gpu, words, gate, eps, mpi, n, slots, stride):
    """One launch on a guarded copy of `words`; returns (words, gate) after it,
    having checked that the guard words before and after the list survive."""
    buf = np.full(FRONT + len(words) + 4, RGUARD, np.uint32)
    buf[FRONT:FRONT + len(words)] = words
    d = torch.from_numpy(buf.view(np.int32)).to(gpu)
    g = torch.from_numpy(np.array(gate, np.uint32).view(np.int32)).to(gpu)
    ops.judge(d[FRONT:], g, eps, mpi, n, slots, stride)
    out = d.cpu().numpy().view(np.uint32)
    assert (out[:FRONT] == RGUARD).all() and (out[FRONT + len(words):] == RGUARD).all()
    return [int(x) for x in out[FRONT:FRONT + len(words)]], \
        [int(x) for x in g.cpu().numpy().view(np.uint32)]


def check_judge(gpu, words, gate, eps, mpi, n=1, slots=1, stride=0):
    want = judge_oracle(words, gate, eps, mpi, n, slots, stride)
    got = run_judge(gpu, words, gate, eps, mpi, n, slots, stride)
    assert got[1] == want[1], (got[1], want[1], dict(eps=eps, mpi=mpi, n=n, slots=slots))
    assert got[0] == want[0]
    return got[1]


def open_gate(checks=5):
    return [0, 0, 0, checks, 0x12345678] + PAD


@pytest.mark.parametrize("mpi", [False, True])
@pytest.mark.parametrize("eps", [1e-3, 0.7, 2.0 ** -10, 0.0])
def test_judge_threshold(gpu, eps, mpi):
    e32 = np.float32(eps)
    rs = [np.nextafter(e32, np.float32(0)), e32, np.nextafter(e32, np.float32(np.inf)),
          np.float32(0.0)]
    got = []
    for r in rs:
        g = check_judge(gpu, [f32_bits(r)], open_gate(), eps, mpi)
        assert g[3] == 6 and g[4] == f32_bits(r)
        assert g[:3] == ([1, 1, 5] if g[0] else [0, 0, 0])
        got.append(bool(g[0]))
    # Worked by hand: float32(1e-3) rounds up, float32(0.7) rounds down, 2^-10
    # is exact; columns: just below e32, e32, just above, 0.
    by_hand = {
        (1e-3, False): [True, False, False, True],
        (1e-3, True): [True, False, False, True],   # e32 > 1e-3 in double
        (0.7, False): [True, False, False, True],
        (0.7, True): [True, True, False, True],     # e32 < 0.7 in double: the modes disagree
        (2.0 ** -10, False): [True, False, False, True],
        (2.0 ** -10, True): [True, True, False, True],
        (0.0, False): [False, False, False, False],  # nothing is < 0
        (0.0, True): [True, True, False, True],      # 0 <= 0; the smallest subnormal is not
    }[(eps, mpi)]
    assert got == by_hand


@pytest.mark.parametrize("mpi", [False, True])
@pytest.mark.parametrize("word", [0x7F800000, 0x7FC00000, 0x7F800001, 0xFFC00000])
def test_judge_nonfinite_words(gpu, word, mpi):
    # eps = 1e30 would accept any finite residual: the exponent test comes first.
    g = check_judge(gpu, [word], open_gate(), 1e30, mpi)
    assert g[:5] == [1, 2, 5, 6, word]
    # in one slot of 64, the others finite (the sign-bit word is the largest
    # unsigned, the others are the largest of their list only as words)
    for slot in (0, 31, 63):
        words = [f32_bits(1.0 + s) for s in range(64)]
        words[slot] = word
        g = check_judge(gpu, words, open_gate(), 1e30, mpi, 1, 64, 1)
        assert g[:5] == [1, 2, 5, 6, word]


def test_judge_closed_gate(gpu):
    rng = np.random.default_rng(3)
    for n, slots, stride in [(1, 1, 0), (33, 2, 38), (70, 64, 70)]:
        words = [int(x) for x in rng.integers(0, 1 << 32, (slots - 1) * stride + n,
                                              dtype=np.uint64)]
        words[0] = 0x7FC00000
        for reason in (1, 2):
            gate = [1, reason, 3, 7, f32_bits(0.25)] + PAD
            g = check_judge(gpu, words, gate, 1e30, False, n, slots, stride)
            assert g == gate  # unchanged; check_judge saw the words zeroed


def _list_case(n, slots, stride, pos, slot, kind, rng):
    """Words of n checks: every check's residual well above eps = 1e-3 except
    the closing one at `pos`, whose deciding word lies in `slot` alone: the
    only non-finite word (kind "nan"; the other slots would not close), or
    the largest of small ones (kind "conv"; last_bits tells).  The check
    after it would close as well, and must not count."""
    words = np.full((slots - 1) * stride + n, RGUARD, np.uint32)
    for s in range(slots):
        vals = (1.0 + rng.random(n)).astype(np.float32)
        if pos is not None:
            if kind == "nan":
                vals[pos] = np.float32(np.nan) if s == slot else vals[pos]
            else:
                vals[pos] = np.float32(9e-4) if s == slot else np.float32(1e-4 * rng.random())
            if pos + 1 < n:
                vals[pos + 1] = np.float32(1e-5)
        words[s * stride:s * stride + n] = vals.view(np.uint32)
    return [int(x) for x in words]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 70])
def test_judge_lists(gpu, n):
    # The kernel takes 32 checks at a time and re-reads the gate for the next
    # 32; lane s reads slot s.  Entry `checks` = 5: ordinals carry on.
    rng = np.random.default_rng(n)
    for slots in (1, 2, 63, 64):
        for stride in (n, n + 5):
            words = _list_case(n, slots, stride, None, 0, "", rng)
            g = check_judge(gpu, words, open_gate(), 1e-3, False, n, slots, stride)
            assert g[:4] == [0, 0, 0, 5 + n]  # no closing check: open, all counted
            for pos in sorted({0, 31, 32, n - 1}):
                if pos >= n:
                    continue
                for slot in sorted({0, slots // 2, slots - 1}):
                    for kind in ("nan", "conv"):
                        words = _list_case(n, slots, stride, pos, slot, kind, rng)
                        g = check_judge(gpu, words, open_gate(), 1e-3, False, n, slots, stride)
                        why = 2 if kind == "nan" else 1
                        assert g[:4] == [1, why, 5 + pos, 5 + pos + 1], (slots, stride, pos, slot)
                        assert g[4] == (words[slot * stride + pos])


def test_judge_argument_checks(gpu):
    r = torch.zeros(256, dtype=torch.int32, device=gpu)
    g = torch.zeros(8, dtype=torch.int32, device=gpu)
    for kw in (dict(n=0), dict(slots=65, stride=1), dict(n=3, slots=2, stride=2)):
        with pytest.raises(_native.NativeError, match="judge of"):
            ops.judge(r, g, 1e-3, **kw)
    with pytest.raises(ValueError):
        ops.judge(r[:10], g, 1e-3, n=8, slots=2, stride=8)  # list longer than the tensor
    with pytest.raises(ValueError):
        ops.judge(r, g[:4], 1e-3)
    torch.cuda.synchronize()
    assert int(r.abs().sum()) == 0 and int(g.abs().sum()) == 0


def test_gate_view(gpu):
    t = ops.Gate(stop=1, reason=2, stop_check=3, checks=4, last_bits=0xFFC00000).tensor(gpu)
    assert t.dtype == torch.int32 and t.numel() == 8
    assert ops.Gate.read(t) == ops.Gate(1, 2, 3, 4, 0xFFC00000)
    r = torch.tensor([f32_bits(0.5)], dtype=torch.int32, device=gpu)
    g = ops.Gate(checks=5).tensor(gpu)
    ops.judge(r, g, 0.7)
    assert ops.Gate.read(g) == ops.Gate(1, 1, 5, 6, f32_bits(0.5)) and int(r[0]) == 0


# ---------------------------------------------------------------------------
# stand-alone residual
# ---------------------------------------------------------------------------
def _pair(lx, ly, gpu, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random((lx, ly), np.float32) * 100).astype(np.float32)
    b = (a + rng.random((lx, ly), np.float32)).astype(np.float32)  # |a - b| < 1
    return a, b


def _residual_word(a, b, gpu, preset=0, box=None):
    fa, fb = SC.field_of(a, gpu), SC.field_of(b, gpu)
    w = torch.tensor([preset, RGUARD], dtype=torch.int64).to(torch.int32).to(gpu)
    ops.residual(fa, fb, box, resid=w)
    out = w.cpu().numpy().view(np.uint32)
    assert out[1] == RGUARD
    return int(out[0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_residual_nonfinite_cell(gpu, bad):
    a, b = _pair(33, 70, gpu, 1)
    b[20, 41] = bad
    w = _residual_word(a, b, gpu)
    assert w & 0x7F800000 == 0x7F800000
    if math.isinf(bad):
        assert w == 0x7F800000
    else:
        assert w & 0x007FFFFF
    # ... which judge turns into reason 2 whatever eps is
    g = check_judge(gpu, [w], open_gate(), 1e30, False)
    assert g[:2] == [1, 2]


def test_residual_word_already_set(gpu):
    a, b = _pair(33, 70, gpu, 2)
    want = f32_bits(np.abs(a - b).max())
    assert _residual_word(a, b, gpu) == want
    assert _residual_word(a, b, gpu, preset=f32_bits(1000.0)) == f32_bits(1000.0)
    assert _residual_word(a, b, gpu, preset=f32_bits(1e-3)) == want
    assert _residual_word(a, b, gpu, preset=0x7FC00000) == 0x7FC00000  # an earlier NaN stays


@pytest.mark.parametrize("lx,ly,at", [
    (4200, 3, (4199, 1)),  # more rows than 4 * 1024: the row stride loops; max in the last row
    (5, 67, (2, 66)),      # columns no multiple of 64; max in column 66
])
def test_residual_stride_edges(gpu, lx, ly, at):
    a, b = _pair(lx, ly, gpu, 3)
    b[at] = a[at] + np.float32(7.0)
    want = f32_bits(np.abs(a - b).max())
    assert want == f32_bits(np.abs(a[at] - b[at]))
    assert _residual_word(a, b, gpu) == want
    # a box that leaves the cell out does not see it
    box = (0, lx - 1, 0, ly) if at[0] == lx - 1 else (0, lx, 0, ly - 1)
    a2, b2 = a[box[0]:box[1], box[2]:box[3]], b[box[0]:box[1], box[2]:box[3]]
    assert _residual_word(a, b, gpu, box=box) == f32_bits(np.abs(a2 - b2).max())
