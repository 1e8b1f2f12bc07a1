"""The stored transpose ("companion", hispmv_set_transposable state HISPMV_TRANSPOSABLE_COMPANION): a handle P created in that state
runs its transposed entries as FORWARD launches over a second, hidden matrix made from the swapped creation input.

Method.  One context per case, under the case's switches.  P is created in state 3 from (r, c, v, rows, cols); R, the reference, in
state 0 from the swapped input (c, r, v, cols, rows); Q in state 2 from P's input (what P is without its companion).  Every y of P's
transposed entries is compared, as int32, with a ONE-VECTOR linear_device call on R with the same x, bias, alpha and beta: equal
bits, whatever the batch around the vector.  Every y lives inside a larger tensor whose other words hold a sentinel that must
survive.  One fp64 scatter truth per case (gate bwd_err < TOL) catches P and R agreeing on a wrong answer.

Inputs (the smallest of tests/step_small_cases.py that reach each mechanism; `T` = the transposed input, so that the COMPANION is the
named matrix).  The formats asserted for 9 - 11 were confirmed with hispmv_prep_choose_format at 256 CUs: tile_stream and
tile_stream_cut_row are tile streams under S.AUTO, stray_split_band is cut in 2 and column_tiled in 8 under S.COLTILES."""
import zlib

import numpy as np
import pytest

import step_small_cases as S
from conftest import TOL
from step_small_harness import HW, SHARED
from util import bwd_err

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5EA15EA1
NV = 7


def T(m):
    return dict(m, name=m["name"] + "_T", rows=m["cols"], cols=m["rows"], r=m["c"], c=m["r"],
                x=np.resize(m["x"], m["rows"]).astype(np.float32), b=np.resize(m["b"], m["cols"]).astype(np.float32))


# name -> (P's input, switches, storage, what the case asserts about the formats)
CASES = {
    "01_one_by_one": (S.one_by_one, S.SLICES, "fp32", {}),
    "02_no_window": (lambda: S.uniform(3000, 2500, 9000, 13, {}), S.SLICES, "fp32", {}),
    "03_window_compact": (lambda: S.uniform(3000, 2500, 600000, 17, {}), S.SLICES, "fp32", dict(window=True)),
    "04_band_cut_rows": (lambda: S.band(4000, 300, 18, {}), S.SLICES, "fp32", dict(window=True)),
    "05_single_row": (S.single_row, S.SLICES, "fp32", {}),
    "06_single_row_T": (lambda: T(S.single_row()), S.SLICES, "fp32", {}),
    "07_sparse_rows_T": (lambda: T(S.sparse_rows()), S.SLICES, "fp32", {}),
    "08_big_band_bf16": (lambda: S.as_bf16(S.big_band()), S.SLICES, "bf16", dict(threads=1024, half=True)),
    "09_tile_stream": (S.tile_stream, S.AUTO, "fp32", dict(format=1)),
    "10_tile_stream_cut_row_T": (lambda: T(S.tile_stream_cut_row()), S.AUTO, "fp32", dict(companion_format=1)),
    "11_two_parts_T": (lambda: T(S.stray_split_band()), S.COLTILES, "fp32", dict(companion_parts=2)),
    "11_eight_parts_T": (lambda: T(S.column_tiled()), S.COLTILES, "fp32", dict(companion_parts=8)),
}
UNALIGNED = ("03_window_compact", "09_tile_stream")
TWICE = ("03_window_compact", "04_band_cut_rows", "06_single_row_T", "11_two_parts_T", "11_eight_parts_T")
UPDATED = ("02_no_window", "03_window_compact", "04_band_cut_rows", "08_big_band_bf16", "09_tile_stream", "11_two_parts_T", "11_eight_parts_T")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def truth(m, x, b, alpha, beta):
    """fp64 scatter of the transposed product and the magnitude sum of its terms."""
    t = m["v"].astype(np.float64) * np.asarray(x, np.float64)[m["r"]]
    bb = beta * np.asarray(b, np.float64)
    return (bb + alpha * np.bincount(m["c"], weights=t, minlength=m["cols"]),
            np.abs(bb) + abs(alpha) * np.bincount(m["c"], weights=np.abs(t), minlength=m["cols"]))


class Trio:
    """P (state 3), a small dense handle D (state 3), R (state 0, swapped input), Q (state 2, P's input) in one context, loaded."""

    def __init__(self, torch, name, updates=False):
        import pyhispmv
        make, env, storage, self.expect = CASES[name]
        self.torch, self.m, self.name = torch, make(), name
        self.dev = torch.device("cuda", 0)
        m = self.m
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.X = rng.random((NV, m["rows"]), dtype=np.float32) - np.float32(0.3)
        self.B = rng.random((NV, m["cols"]), dtype=np.float32)
        self._refs = {}
        with S.environment(dict(SHARED, **env)):
            self.h = h = pyhispmv.FpgaHandle(*HW)
            try:
                h.set_value_storage(storage)
                h.set_value_updates(("any_storage" if storage == "bf16" else True) if updates else False)
                h.set_transposable("companion")
                self.P = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
                self.D = h.create_dense_handle(np.arange(12, dtype=np.float32), 3, 4)
                h.set_transposable(0)
                self.R = h.create_sparse_handle(m["c"], m["r"], m["v"], m["cols"], m["rows"])
                h.set_transposable("keep_format")
                self.Q = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
                assert (self.P, self.D, self.R, self.Q) == (0, 1, 2, 3) and h.num_matrices() == 4
                h.load_matrices()
            except BaseException:
                h.close()
                raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.h.close()

    def device(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def framed(self, n, fill=None):
        """A device tensor of n floats (NaN, or `fill`) between two guards of sentinel words -> (tensor, pointer of the n floats)."""
        Y0 = np.full(n + 2 * GUARD, SENTINEL, np.int32).view(np.float32)
        Y0[GUARD:GUARD + n] = np.nan if fill is None else np.asarray(fill, np.float32).reshape(-1)
        d = self.device(Y0)
        return d, d.data_ptr() + 4 * GUARD

    def unframe(self, d, n):
        self.h.synchronize()
        out = d.cpu().numpy()
        guard = np.ones(out.size, bool)
        guard[GUARD:GUARD + n] = False
        assert (out.view(np.int32)[guard] == SENTINEL).all(), f"{self.name}: words outside y were written"
        return out[GUARD:GUARD + n].copy()

    def ref(self, x, b, alpha, beta):
        """The reference route: a one-vector linear_device call on R (the fix-up carry variant); computed once per argument set."""
        key = (bits(x).tobytes(), None if b is None else bits(b).tobytes(), alpha, beta)
        if key not in self._refs:
            n = self.m["cols"]
            dx, db = self.device(x), (self.device(b) if b is not None else None)
            dy, py = self.framed(n)
            self.torch.cuda.synchronize()
            self.h.linear_device(self.R, dx.data_ptr(), 1, db.data_ptr() if db is not None else 0, py, alpha, beta)
            self._refs[key] = self.unframe(dy, n)
        return self._refs[key]

    def spmv_t(self, x, b, alpha, beta):
        n = self.m["cols"]
        dx, db = self.device(x), (self.device(b) if b is not None else None)
        dy, py = self.framed(n)
        self.torch.cuda.synchronize()
        self.h.spmv_device_t(self.P, dx.data_ptr(), db.data_ptr() if db is not None else 0, py, alpha, beta)
        return self.unframe(dy, n)

    def linear_t(self, nv, mode, alpha=1.0, beta=1.0, shift_x=0):
        """linear_device_t on P with the first nv vectors -> y [nv, cols].  mode: "beta0" (NULL bias), "shared" (bias_stride 0),
        "per_vector" (bias_stride cols, its own buffer), "in_place" (bias_stride cols, d_bias == d_y).  shift_x: floats by which d_x is
        moved off the 16-byte alignment."""
        m = self.m
        n = nv * m["cols"]
        dx = self.device(np.concatenate([np.zeros(shift_x, np.float32), self.X[:nv].reshape(-1)]))
        dy, py = self.framed(n, fill=self.B[:nv] if mode == "in_place" else None)
        db = self.device(self.B[:nv] if mode == "per_vector" else self.B[0])
        pb, stride = {"beta0": (0, 0), "shared": (db.data_ptr(), 0), "per_vector": (db.data_ptr(), m["cols"]), "in_place": (py, m["cols"])}[mode]
        self.torch.cuda.synchronize()
        self.h.linear_device_t(self.P, dx.data_ptr() + 4 * shift_x, nv, pb, py, alpha, 0.0 if mode == "beta0" else beta, bias_stride=stride)
        return self.unframe(dy, n).reshape(nv, m["cols"])

    def linear_t_refs(self, nv, mode, alpha=1.0, beta=1.0):
        if mode == "beta0":
            return np.stack([self.ref(self.X[v], None, alpha, 0.0) for v in range(nv)])
        return np.stack([self.ref(self.X[v], self.B[0 if mode == "shared" else v], alpha, beta) for v in range(nv)])

    def forward(self, k, x, b, alpha, beta):
        dx, db = self.device(x), self.device(b)
        dy, py = self.framed(self.m["rows"])
        self.torch.cuda.synchronize()
        self.h.spmv_device(k, dx.data_ptr(), db.data_ptr(), py, alpha, beta)
        return self.unframe(dy, self.m["rows"])

    def update(self, v):
        dv = self.device(v)
        self.torch.cuda.synchronize()
        for k in (self.P, self.R, self.Q):
            self.h.update_values_device(k, dv.data_ptr(), v.size)
        self.h.synchronize()
        self._refs.clear()


def check_formats(cx):
    h, e = cx.h, cx.expect
    ip, ir, ci = h.matrix_info(cx.P), h.matrix_info(cx.R), h.companion_info(cx.P)
    print(f"{cx.name}: P {ip['format']}/{ip['col_tiles']} parts, companion {ci}, R {ir['format']}/{ir['col_tiles']} parts, "
          f"{ir['block_threads']} threads, window {ir['lds_bytes']} B")
    assert ci["has"] and ci["format"] == ir["format"] and ci["parts"] == ir["col_tiles"] and ci["tile_kind"] == ir["tile_kind"], (ci, ir)
    if "format" in e:
        assert ip["format"] == e["format"], ip
    if "companion_format" in e:
        assert ci["format"] == e["companion_format"], ci
    if "companion_parts" in e:
        assert ci["parts"] == e["companion_parts"] and ci["parts"] > 1, ci
    if "window" in e:
        assert (ir["lds_bytes"] > 0) == e["window"], ir
    if "threads" in e:
        assert ir["block_threads"] == e["threads"], ir
    if e.get("half"):
        assert h.value_storage_info(cx.R)["slots_2byte"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_transposed_entries_have_the_bits_of_the_swapped_handle(torch_mod, name):
    with Trio(torch_mod, name) as cx:
        h, m = cx.h, cx.m
        check_formats(cx)
        # ---- info
        ti = h.transpose_info(cx.P)
        assert ti["transposable"] and ti["atomic_bytes"] == 0 and ti["direct_elems"] == 0 and ti["launches"] >= 1, ti
        lp, lr = h.linear_info(cx.P, NV), h.linear_info(cx.R, NV)
        assert (lp["width_t"], lp["passes_t"]) == (lr["width"], lr["passes"]) and lp["launches_t"] >= lp["passes_t"], (lp, lr)
        ci = h.companion_info(cx.P)
        assert not h.companion_info(cx.R)["has"] and not h.companion_info(cx.D)["has"] and not h.companion_info(cx.Q)["has"]
        assert h.companion_info(cx.D) == dict(has=False, format=0, parts=0, device_bytes=0, map_slots=0, tile_kind=0)
        assert ci["device_bytes"] > 0 and ci["map_slots"] == 0
        assert h.matrix_info(cx.P)["device_bytes"] == h.matrix_info(cx.Q)["device_bytes"] + ci["device_bytes"]
        # ---- one vector
        x, b = cx.X[0], cx.B[0]
        y = cx.spmv_t(x, None, 1.0, 0.0)
        assert np.array_equal(bits(y), bits(cx.ref(x, None, 1.0, 0.0)))
        y = cx.spmv_t(x, b, 0.75, -1.5)
        assert np.array_equal(bits(y), bits(cx.ref(x, b, 0.75, -1.5)))
        y64, mag = truth(m, x, b, 0.75, -1.5)
        err = bwd_err(y, y64, mag)
        print(f"{name}: backward error against the fp64 scatter {err:.3e}")
        assert np.isfinite(y).all() and err < TOL, err
        y = cx.spmv_t(np.full(m["rows"], np.nan, np.float32), b, 0.0, 2.0)      # alpha == 0: x is not read
        assert np.array_equal(bits(y), bits(np.float32(2.0) * b))
        # ---- several vectors: every vector has the bits of its one-vector reference, whatever num_vecs
        for mode in ("beta0", "shared", "per_vector", "in_place"):
            want = cx.linear_t_refs(NV, mode)
            for nv in (1, 2, 3, 4, 7):
                got = cx.linear_t(nv, mode)
                bad = [v for v in range(nv) if not np.array_equal(bits(got[v]), bits(want[v]))]
                assert not bad, (name, mode, nv, bad)
        if name in UNALIGNED:
            got = cx.linear_t(4, "shared", shift_x=1)
            assert np.array_equal(bits(got), bits(cx.linear_t_refs(4, "shared")))
        if name in TWICE:
            first, second = cx.linear_t(NV, "shared", 0.75, -1.5), cx.linear_t(NV, "shared", 0.75, -1.5)
            assert np.array_equal(bits(first), bits(second))
            assert np.array_equal(bits(first), bits(cx.linear_t_refs(NV, "shared", 0.75, -1.5)))
        # ---- the forward product is that of the handle without a companion
        assert np.array_equal(bits(cx.forward(cx.P, m["x"], m["b"], 0.85, -2.06)), bits(cx.forward(cx.Q, m["x"], m["b"], 0.85, -2.06)))


def new_values(cx, seed):
    v = (np.random.default_rng(seed).random(cx.m["v"].size, dtype=np.float32) - np.float32(0.5)) * np.float32(3.0)
    return S.bf16_exact(v) if cx.m.get("storage") == "bf16" else v


def check_after_update(cx, v2):
    """Both products of P after an update: the transposed one has the bits of R's forward (and is the product of the NEW values), the
    forward one those of Q's."""
    m = cx.m
    x, b = cx.X[0], cx.B[0]
    y = cx.spmv_t(x, b, 0.75, -1.5)
    assert np.array_equal(bits(y), bits(cx.ref(x, b, 0.75, -1.5)))
    y64, mag = truth(dict(m, v=v2), x, b, 0.75, -1.5)
    old64, _ = truth(m, x, b, 0.75, -1.5)
    assert bwd_err(y, y64, mag) < TOL and bwd_err(y, old64, mag) > 100 * TOL
    for mode in ("beta0", "in_place"):
        assert np.array_equal(bits(cx.linear_t(3, mode)), bits(cx.linear_t_refs(3, mode))), mode
    assert np.array_equal(bits(cx.forward(cx.P, m["x"], m["b"], 0.85, -2.06)), bits(cx.forward(cx.Q, m["x"], m["b"], 0.85, -2.06)))


@pytest.mark.parametrize("name", UPDATED)
def test_one_update_reaches_both_matrices(torch_mod, name):
    with Trio(torch_mod, name, updates=True) as cx:
        h, m = cx.h, cx.m
        check_formats(cx)
        up, uq, ci = h.value_update_info(cx.P), h.value_update_info(cx.Q), h.companion_info(cx.P)
        assert up["updatable"] and up["n"] == m["v"].size == uq["n"], (up, uq)
        assert ci["map_slots"] >= m["v"].size and up["written"] >= uq["written"] + ci["map_slots"], (up, uq, ci)
        assert h.matrix_info(cx.P)["device_bytes"] == h.matrix_info(cx.Q)["device_bytes"] + ci["device_bytes"]
        # the load's own update: the creation values are in both
        y = cx.spmv_t(cx.X[0], cx.B[0], 0.75, -1.5)
        assert np.array_equal(bits(y), bits(cx.ref(cx.X[0], cx.B[0], 0.75, -1.5)))
        v2 = new_values(cx, 77)
        cx.update(v2)
        check_after_update(cx, v2)
        # the value gradient reads only the primary
        gy, gx = cx.device(cx.X[:3]), cx.device(cx.B[:3])           # [3, rows] and [3, cols]
        grads = []
        for k in (cx.P, cx.Q):
            dg, pg = cx.framed(m["v"].size)
            torch_mod.cuda.synchronize()
            h.value_grad_device(k, gy.data_ptr(), gx.data_ptr(), 3, pg)
            grads.append(cx.unframe(dg, m["v"].size))
        assert np.array_equal(bits(grads[0]), bits(grads[1])) and np.isfinite(grads[0]).all()
        if name == "02_no_window":          # the host entry writes both as well
            v3 = new_values(cx, 78)
            for k in (cx.P, cx.R, cx.Q):
                h.update_values(k, v3)
            cx._refs.clear()
            check_after_update(cx, v3)


def test_csr_input_keeps_its_value_order(torch_mod):
    """A handle from CSR with unsorted rows, in state 3 and updatable: the companion is made from the swapped COO in input order, so an
    update in that order reaches the same entries of both; R is created from that swapped COO."""
    import pyhispmv
    m = S.uniform(3000, 2500, 9000, 13, {})
    rng = np.random.default_rng(5)
    order = np.lexsort((rng.random(m["r"].size), m["r"]))           # rows ascending, columns in random order inside a row
    r, c, v = m["r"][order], m["c"][order], m["v"][order]
    rp = np.zeros(m["rows"] + 1, np.int64)
    np.add.at(rp, r.astype(np.int64) + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    x = rng.random(m["rows"], dtype=np.float32)
    with S.environment(dict(SHARED, **S.SLICES)):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_value_updates(True)
        h.set_transposable("companion")
        P = h.create_sparse_handle_from_csr(rp, c, v, m["rows"], m["cols"])
        h.set_transposable(0)
        R = h.create_sparse_handle(c, r, v, m["cols"], m["rows"])
        h.load_matrices()
        assert h.companion_info(P)["has"] and h.value_update_info(P)["n"] == v.size
        dx = torch_mod.from_numpy(x).cuda()
        for values in (None, (rng.random(v.size, dtype=np.float32) - np.float32(0.5))):
            if values is not None:
                dv = torch_mod.from_numpy(values).cuda()
                torch_mod.cuda.synchronize()
                h.update_values_device(P, dv.data_ptr(), v.size)
                h.update_values_device(R, dv.data_ptr(), v.size)
            yp = torch_mod.full((m["cols"],), float("nan"), device="cuda")
            yr = torch_mod.full((m["cols"],), float("nan"), device="cuda")
            torch_mod.cuda.synchronize()
            h.spmv_device_t(P, dx.data_ptr(), 0, yp.data_ptr(), 1.0, 0.0)
            h.linear_device(R, dx.data_ptr(), 1, 0, yr.data_ptr(), 1.0, 0.0)
            h.synchronize()
            yp, yr = yp.cpu().numpy(), yr.cpu().numpy()
            assert np.array_equal(bits(yp), bits(yr))
            y64, mag = truth(dict(m, r=r, c=c, v=v if values is None else values), x, np.zeros(m["cols"]), 1.0, 0.0)
            assert bwd_err(yp, y64, mag) < TOL
    finally:
        torch_mod.cuda.synchronize()
        h.close()


def test_arena_counts_both_and_a_refusal_leaves_no_trace(torch_mod):
    """Input 3: the arena is sized so that the primary fits and primary + companion does not.  Creation in state 3 returns -1 and the
    context is as before; the same input then fits in state 2; with room, state 3 registers one handle that costs the sum."""
    import pyhispmv
    m = S.uniform(3000, 2500, 600000, 17, {})
    with S.environment(dict(SHARED, **S.SLICES)):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_transposable("keep_format")
        q0 = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        primary = h.matrix_info(q0)["device_bytes"]
        used = h.arena_bytes_used()
        assert q0 == 0 and used == primary > 0
        h.set_arena_bytes(used + primary + 4096)
        h.set_transposable("companion")
        assert h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"]) == -1
        assert h.num_matrices() == 1 and h.arena_bytes_used() == used
        h.set_transposable("keep_format")
        assert h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"]) == 1
        assert h.arena_bytes_used() == 2 * primary
        h.set_arena_bytes(1 << 40)
        h.set_transposable("companion")
        p = h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        ci = h.companion_info(p)
        assert p == 2 and h.num_matrices() == 3 and ci["has"] and ci["device_bytes"] > 4096
        assert h.matrix_info(p)["device_bytes"] == primary + ci["device_bytes"]
        assert h.arena_bytes_used() == 3 * primary + ci["device_bytes"]
        h.load_matrices()
        assert h.transpose_info(p)["transposable"] and h.transpose_info(p)["atomic_bytes"] == 0 and h.transpose_info(q0)["atomic_bytes"] > 0
    finally:
        h.close()


@pytest.mark.parametrize("env", [dict(S.TTS, HISPMV_TTS_GEOMETRY="tall"), S.TTS_SMALL], ids=["tall", "small"])
def test_experimental_tile_geometries_are_refused_at_creation(torch_mod, env):
    import pyhispmv
    m = S.uniform(3000, 2500, 9000, 13, {})
    with S.environment(dict(SHARED, **env)):
        h = pyhispmv.FpgaHandle(*HW)
    try:
        h.set_transposable("companion")
        with pytest.raises(ValueError, match="HISPMV_TTS_GEOMETRY"):
            h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"])
        assert h.num_matrices() == 0 and h.arena_bytes_used() == 0
        assert h.create_dense_handle(np.arange(12, dtype=np.float32), 3, 4) == 0          # dense handles ignore the state
        h.set_transposable("keep_format")
        assert h.create_sparse_handle(m["r"], m["c"], m["v"], m["rows"], m["cols"]) == 1
    finally:
        h.close()


def test_no_free_was_rejected():
    from hispmv_amd._lib import lib
    assert lib.hispmv_free_failures() == 0
