"""The scheduling layer above the validity kernels (launch_validity, nbk_validity_batch, nbk_edge_validity_batch): batch
tiling, odd tiles on the library's second stream with its own scratch set (cached tables, two counter sets, overflow marks, world
epoch), and narrowphase chunks handed out by ticket.  ``pipe_tile = 16384`` brings the two-stream pipeline down from 2^21 rows to
32 768, so every row of every call is compared with the oracle -- exactly, there is no tolerance in this file -- and
``DeviceModel.last_tiling`` says whether a call really was pipelined.  Needs a real MI355X."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.cpu_oracle import Oracle
from numbotics_amd import _lib
from numbotics_amd._lib import debug_option
from numbotics_amd.parallel import unpack_mask
from numbotics_amd.scenes import sample_q
from test_gpu_parity import torch_cuda, assert_bitwise      # noqa: F401  (fixture)
from test_gpu_world_poses import pose_sets
from test_world_poses_host import world_scene

TILE = 16384                                    # NSUB * 64: the smallest tile the library accepts
# just below the switch | exactly two tiles | three tiles, the last of one row | four tiles: each scratch set is used twice, the
# second time through its cached tables | six tiles, a 17-row tail, and >= 65 536 plain rows (the per-robot broadphase on c2)
BATCHES = (32767, 32768, 32769, 65536, 81937)
BMAX = BATCHES[-1]
THRESHOLDS = (0.0, 1e-6, 0.02, -0.005)
NO_JIT = os.environ.get("NBK_NO_JIT", "0") not in ("", "0")


def tiling(B, tile=TILE, on=True):
    """(tiles, rows per tile, pipelined) of a call of B rows: pipelined from two tiles on, else one tile of B rounded up to 64."""
    if on and B >= 2 * tile:
        return (-(-B // tile), tile, 1)
    return (1, (B + 63) // 64 * 64, 0)


def assert_tiles_mixed(ref, what):
    """Both verdicts in every full tile of the reference: a tile that came back all zero or all one cannot pass."""
    full = ref[: len(ref) // TILE * TILE].reshape(-1, TILE)
    assert len(full) >= 1 and full.any(axis=1).all() and (~full).any(axis=1).all(), what


def words_of(mask):
    """(B,) bool -> the packed words nbk_validity_batch writes for it (bits at and above B are zero)."""
    by = np.packbits(mask, bitorder="little")
    out = np.zeros(((len(mask) + 63) // 64) * 8, dtype=np.uint8)
    out[: len(by)] = by
    return out.view(np.int64)


class Case:
    """One scene on the device, BMAX rows of q (``sample_q(chain, 81937, seed=11)``) and their oracle masks, one per threshold,
    computed once and never written to."""

    def __init__(self, torch, scene, margins=True, thresholds=THRESHOLDS, **arm_kw):
        self.torch = torch
        self.arm, self.chain, self.obs = world_scene(scene, bullet_margins=margins, **arm_kw)
        self.sm = self.arm.scene_model()
        self.dev = self.arm._scene_device()[1]
        self.orc = Oracle(self.sm)
        self.q = sample_q(self.chain, BMAX, seed=11)
        self.qt = torch.from_numpy(self.q).cuda()
        self.ref = {}
        for thr in thresholds:
            r = self.orc.validity(self.q, thr, nthreads=8)
            r.setflags(write=False)
            assert_tiles_mixed(r, (scene, margins, thr))
            self.ref[thr] = r

    def raw(self, q, B, thr, words=None, mask=None, stream=None):
        """nbk_validity_batch itself -> status."""
        torch = self.torch
        st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        return self.dev._lib.nbk_validity_batch(self.dev._h, q.data_ptr(), B, float(thr), None if words is None else words.data_ptr(),
                                                None if mask is None else mask.data_ptr(), st)

    def check(self, B, thr, what, packed=False, expect=None):
        """One call on q[:B] against the oracle, and what the library says about its tiling."""
        got = self.dev.validity(self.qt[:B], thr, packed=packed).cpu().numpy()
        if expect is not None:
            assert self.dev.last_tiling() == expect, (what, self.dev.last_tiling(), expect)
        if packed:
            assert np.array_equal(got, words_of(self.ref[thr][:B])), (what, "words")
        else:
            bad = np.nonzero(got != self.ref[thr][:B])[0]
            assert bad.size == 0, f"{what}: {bad.size} of {B} rows differ from the oracle, first at {bad[:8]} (tiles {bad[:8] // TILE})"
        return got


def test_no_pipeline_below_two_tiles_at_the_default_size(fresh_world, torch_cuda):
    """At the default tile of 2^20 rows none of this file's batches is pipelined: the diagnostic says so, and reports nothing
    before the first two-kernel launch."""
    c = Case(torch_cuda, "c2", thresholds=(0.0,))
    assert c.dev.last_tiling() == (0, 0, 0)
    c.check(BMAX, 0.0, "default pipe_tile", expect=tiling(BMAX, on=False))
    with debug_option("two_kernel_min_b", 10 ** 9):                    # the fused kernel is no two-kernel launch
        c.dev.validity(c.qt[:4096], 0.0)
    assert c.dev.last_tiling() == tiling(BMAX, on=False)


MASK_SCENES = ("c2", "c3", "c5m")
MASK_MARGINS = (True, False)


def expected_narrow_builds(scene, margins):
    """The narrowphase builds a case of test_masks_on_every_build_and_broadphase may launch, per threshold of THRESHOLDS, from the
    contact threshold tc = (thr + mA) + mB of the pairs that reach GJK.  Sharp boxes, cylinders and hulls have margin 0, so tc =
    thr in the primitive scenes (the arm's one sphere reaches GJK against hulls only): zero -> the boolean walk alone, positive
    -> k_narrow_pos, negative -> k_narrow_pred.  Bullet margins are > 0 on boxes, cylinders and hulls, so tc > 0 at thr >= 0.
    The mesh scene always needs the distance iteration for its hulls (k_narrow_pos at thr >= 0), and at -0.005 it mixes signs in
    both modes, which is the full k_narrow: hull against hull has tc = -0.005 (sharp) or 0.002 - 0.005 (Bullet), the 0.03 m
    sphere, whose radius is its margin, against a hull has tc >= 0.03 - 0.005.  The Bullet primitive scenes at -0.005 have sums
    of margins on both sides of 0.005 or only above it, depending on the pair list: either build."""
    hulls = scene == "c5m"
    if hulls:
        return [{"k_narrow_pos"}] * 3 + [{"k_narrow"}]
    if not margins:
        return [{"k_narrow_bool"}, {"k_narrow_pos"}, {"k_narrow_pos"}, {"k_narrow_pred"}]
    return [{"k_narrow_pos"}] * 3 + [{"k_narrow_pos", "k_narrow"}]


def test_parametrisation_reaches_all_four_narrow_builds():
    """The scenes, margin modes and thresholds of test_masks_on_every_build_and_broadphase between them launch k_narrow_bool,
    k_narrow_pos, k_narrow_pred and k_narrow: counted over the cases whose build is certain (each case checks its own against
    the device)."""
    from numbotics_amd.engine import DeviceModel
    certain = set()
    for scene in MASK_SCENES:
        for margins in MASK_MARGINS:
            certain |= {next(iter(b)) for b in expected_narrow_builds(scene, margins) if len(b) == 1}
    assert certain == set(DeviceModel.NARROW_BUILDS)


@pytest.mark.parametrize("margins", MASK_MARGINS, ids=["bullet", "sharp"])
@pytest.mark.parametrize("scene", MASK_SCENES)
def test_masks_on_every_build_and_broadphase(fresh_world, scene, margins, torch_cuda):
    """Byte masks, packed words and both at once at every batch size of the table, four thresholds; the float64 and the LDS
    broadphase, and the same batch with the pipeline switched off.  c5m's hulls take the LDS-staged vertices of the narrowphase
    and the hull form of the broadphase."""
    torch = torch_cuda
    c = Case(torch, scene, margins)
    assert (c.sm.n_hulls > 0) == (scene == "c5m")
    for thr, allowed in zip(THRESHOLDS, expected_narrow_builds(scene, margins)):
        assert c.dev.narrow_build(thr) in allowed, (scene, margins, thr, c.dev.narrow_build(thr))
    with debug_option("pipe_tile", TILE):
        for thr in THRESHOLDS:
            for B in BATCHES:
                what = f"{scene} {'bullet' if margins else 'sharp'} thr={thr} B={B}"
                c.check(B, thr, what, packed=False, expect=tiling(B))
                c.check(B, thr, what, packed=True, expect=tiling(B))
            if scene == "c2":
                assert c.dev.broad_kernel_used() == (1 if NO_JIT else 2)          # BMAX plain rows: the per-robot kernel
            # bits and bytes from one call
            words = torch.full(((BMAX + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            mask = torch.full((BMAX,), 0xAB, dtype=torch.uint8, device="cuda")
            assert c.raw(c.qt, BMAX, thr, words, mask) == 0
            assert c.dev.last_tiling() == tiling(BMAX)
            assert np.array_equal(mask.cpu().numpy(), c.ref[thr].astype(np.uint8)), (scene, thr, "bytes of the two-output call")
            assert np.array_equal(words.cpu().numpy(), words_of(c.ref[thr])), (scene, thr, "words of the two-output call")
        piped = {thr: c.check(BMAX, thr, "pipelined words", packed=True, expect=tiling(BMAX)) for thr in THRESHOLDS}
        for thr in THRESHOLDS:
            with debug_option("f64_broad", 1):
                c.check(BMAX, thr, f"{scene} thr={thr} float64 broadphase", expect=tiling(BMAX))
                if scene == "c2":
                    assert c.dev.broad_kernel_used() == 3
                c.check(65536, thr, f"{scene} thr={thr} float64 broadphase", packed=True, expect=tiling(65536))
            with debug_option("no_reg_broad", 1):
                c.check(BMAX, thr, f"{scene} thr={thr} LDS broadphase", expect=tiling(BMAX))
                c.check(32769, thr, f"{scene} thr={thr} LDS broadphase", packed=True, expect=tiling(32769))
            with debug_option("pipeline_tiles", 0):
                serial = c.check(BMAX, thr, f"{scene} thr={thr} pipeline off", packed=True, expect=tiling(BMAX, on=False))
            assert np.array_equal(serial, piped[thr]), (scene, thr, "the pipeline changed the words")


def test_every_output_byte_is_the_calls_own(fresh_world, torch_cuda):
    """Whatever the output buffers held before: the words come back identical (the last word's bits at and above B included),
    their bits below B are the oracle's, and every byte is 0 or 1."""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=(0.0, 0.02))
    with debug_option("pipe_tile", TILE):
        for thr in (0.0, 0.02):
            for B in (32769, 65536, BMAX):
                nw = (B + 63) // 64
                runs = []
                for fill in (-1, 0):
                    words = torch.full((nw + 2,), fill, dtype=torch.int64, device="cuda")       # two guard words behind the mask
                    mask = torch.full((B + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                    assert c.raw(c.qt, B, thr, words, mask) == 0
                    assert c.dev.last_tiling() == tiling(B)
                    w, m = words.cpu().numpy(), mask.cpu().numpy()
                    assert (w[nw:] == fill).all() and (m[B:] == 0xAB).all(), (thr, B, "wrote past the outputs")
                    assert np.isin(m[:B], (0, 1)).all() and np.array_equal(m[:B].astype(bool), c.ref[thr][:B]), (thr, B, fill)
                    assert np.array_equal(unpack_mask(w[:nw], B), c.ref[thr][:B]), (thr, B, fill)
                    runs.append(w[:nw])
                assert np.array_equal(runs[0], runs[1]), (thr, B, "words depend on what the buffer held")
                assert np.array_equal(runs[0], words_of(c.ref[thr][:B])), (thr, B)
                # packed output alone, bytes alone
                for fill in (-1, 0):
                    words = torch.full((nw,), fill, dtype=torch.int64, device="cuda")
                    assert c.raw(c.qt, B, thr, words, None) == 0
                    assert np.array_equal(words.cpu().numpy(), runs[0]), (thr, B, fill, "words alone")
                mask = torch.full((B,), 0xAB, dtype=torch.uint8, device="cuda")
                assert c.raw(c.qt, B, thr, None, mask) == 0
                assert np.array_equal(mask.cpu().numpy(), c.ref[thr][:B].astype(np.uint8)), (thr, B, "bytes alone")


def test_the_switch_changes_nothing(fresh_world, torch_cuda):
    """Any value of pipe_tile is rounded down to whole 64-row blocks and raised to 16 384 rows; with that tile, or with the
    pipeline off, the words are the same."""
    c = Case(torch_cuda, "c2", thresholds=(0.0, 0.02))
    B2 = 6 * TILE + 17
    q2 = sample_q(c.chain, B2, seed=12)
    q2t = c.torch.from_numpy(q2).cuda()
    ref2 = c.orc.validity(q2, 0.02, nthreads=8)
    assert_tiles_mixed(ref2, "seed 12")
    ref2 = words_of(ref2)
    for thr in (0.0, 0.02):
        want = words_of(c.ref[thr])
        for value in (1, 1000, TILE + 37, 3 * TILE + 1):
            tile = max(value // 64 * 64, TILE)
            assert tile == (TILE if value < 3 * TILE else 3 * TILE)
            for on in (1, 0):
                with debug_option("pipe_tile", value), debug_option("pipeline_tiles", on):
                    got = c.dev.validity(c.qt, thr, packed=True).cpu().numpy()
                    assert c.dev.last_tiling() == tiling(BMAX, tile, on=bool(on)), (value, on, c.dev.last_tiling())
                    assert np.array_equal(got, want), (thr, value, on)
    # 3 x 16384 + 1 -> tiles of 49 152 rows: BMAX is less than two of them, 98 321 rows are two and a 17-row third
    assert tiling(BMAX, 3 * TILE) == (1, 81984, 0) and tiling(B2, 3 * TILE) == (3, 3 * TILE, 1)
    with debug_option("pipe_tile", 3 * TILE + 1):
        got = c.dev.validity(q2t, 0.02, packed=True).cpu().numpy()
        assert c.dev.last_tiling() == (3, 3 * TILE, 1)
    assert np.array_equal(got, ref2)
    with debug_option("pipe_tile", TILE):
        got = c.dev.validity(q2t, 0.02, packed=True).cpu().numpy()
        assert c.dev.last_tiling() == (7, TILE, 1)
    assert np.array_equal(got, ref2)


@pytest.mark.parametrize("B", [32769, BMAX])
def test_non_finite_rows_at_the_seams(fresh_world, B, torch_cuda):
    """NaN / inf in the last row of tile 0, the first row of tile 1, the first row of the last tile and the last row of the batch:
    those rows collide, every other row is the oracle's."""
    torch = torch_cuda
    c = Case(torch, "c2", thresholds=(0.0,))
    n_tiles = -(-B // TILE)
    rows = [TILE - 1, TILE, (n_tiles - 1) * TILE, B - 1]
    q = c.q[:B].copy()
    for k, (r, v) in enumerate(zip(rows, (np.nan, np.inf, -np.inf, np.nan))):
        q[r, (2 * k) % q.shape[1]] = v
    qt = torch.from_numpy(q).cuda()
    for thr in (0.0, 0.02):
        ref = c.orc.validity(q, thr, nthreads=8)
        assert ref[rows].all()
        others = np.ones(B, dtype=bool)
        others[rows] = False
        assert np.array_equal(ref[others], c.orc.validity(c.q[:B], thr, nthreads=8)[others])
        with debug_option("pipe_tile", TILE):
            got = c.dev.validity(qt, thr).cpu().numpy()
            assert c.dev.last_tiling() == tiling(B)
            words = c.dev.validity(qt, thr, packed=True).cpu().numpy()
            for flag in ("f64_broad", "no_reg_broad"):
                with debug_option(flag, 1):
                    assert np.array_equal(c.dev.validity(qt, thr).cpu().numpy(), ref), (thr, flag)
                    assert c.dev.last_tiling() == tiling(B)
        assert got[rows].all() and np.array_equal(got, ref), (thr, np.nonzero(got != ref)[0][:8])
        assert np.array_equal(words, words_of(ref)), thr


def test_state_across_pipelined_calls(fresh_world, torch_cuda):
    """Both scratch sets keep tables for THEIR last threshold and alternate two counter sets: repeats, a threshold change, a
    small unpipelined call in between, a larger batch (the second stream's set regrows), an edge batch on the same scratch, the
    pipeline switched off and on again -- one stream, every result against the oracle."""
    c = Case(torch_cuda, "c3", thresholds=(0.0, 0.02, -0.005))
    s, g = c.q[:300], c.q[300:600]
    e_ref = c.orc.edge_validity(s, g, 0.05, 1.5)
    with debug_option("pipe_tile", TILE):
        c.check(32769, 0.0, "1: pipelined at 0.0", expect=tiling(32769))
        c.check(32769, 0.0, "2: again (cached tables on both streams)", packed=True, expect=tiling(32769))
        c.check(9000, 0.02, "3: small, unpipelined, at 0.02", expect=tiling(9000))
        c.check(BMAX, 0.02, "4: pipelined at 0.02, larger", expect=tiling(BMAX))
        ok, end, ns = c.dev.edge_validity(s, g, 0.05, 1.5)
        assert np.array_equal(ok, e_ref[0]) and np.array_equal(ns, e_ref[2]), "5: edge batch"
        assert_bitwise(end, e_ref[1], "5: edge ends")
        c.check(BMAX, -0.005, "6: pipelined at -0.005", packed=True, expect=tiling(BMAX))
        with debug_option("pipeline_tiles", 0):
            c.check(BMAX, -0.005, "7: pipeline off, same size", expect=tiling(BMAX, on=False))
        c.check(BMAX, 0.0, "8: pipelined at 0.0", expect=tiling(BMAX))
        c.check(65536, 0.0, "9: pipelined at 0.0, smaller", packed=True, expect=tiling(65536))


def test_call_keeps_its_place_in_the_stream(fresh_world, torch_cuda):
    """"Begins after, and completes before, its neighbours": on a side stream, with no host synchronisation, q (all NaN) is
    filled by a copy right before the call and wiped with NaN right after its result was cloned.  An odd tile that started early or
    finished late would read NaN rows and report them colliding, and a clone taken before an odd tile finished holds the 0xAB the
    mask was filled with.  Each round first queues some milliseconds of unrelated device work on the side stream, so that the host
    has issued the whole round before the device reaches the copy: whatever the library does not order is then free to overlap.
    Without that backlog the device finishes each short step before the host issues the next, and nothing could be seen.  (A race
    check: it can pass by luck, never fail on correct code.)"""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=(0.0,))
    sizes = (BMAX, 65536, BMAX)                  # the last odd tile: a 17-row tail, a full tile
    srcs = [c.q] + [sample_q(c.chain, BMAX, seed=20 + k) for k in range(2)]
    refs = [c.ref[0.0]] + [c.orc.validity(s, 0.0, nthreads=8) for s in srcs[1:]]
    for r in refs:
        assert_tiles_mixed(r, "stream order")
    src_t = [torch.from_numpy(s).cuda() for s in srcs]
    q = torch.full((BMAX, c.dev.n_q), float("nan"), dtype=torch.float64, device="cuda")
    mask = torch.empty((BMAX,), dtype=torch.uint8, device="cuda")
    ballast = torch.zeros((1 << 26,), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    with debug_option("pipe_tile", TILE), torch.cuda.stream(side):
        for k in range(3):
            for _ in range(100):
                ballast.add_(1.0)
            mask.fill_(0xAB)
            q.copy_(src_t[k])
            assert c.raw(q, sizes[k], 0.0, None, mask, stream=side) == 0
            assert c.dev.last_tiling() == tiling(sizes[k])
            outs.append(mask.clone())
            q.fill_(float("nan"))
        side.synchronize()
    for k in range(3):
        got = outs[k].cpu().numpy()
        assert (got[sizes[k]:] == 0xAB).all()
        bad = np.nonzero(got[: sizes[k]] != refs[k][: sizes[k]].astype(np.uint8))[0]
        assert bad.size == 0, f"round {k}: {bad.size} rows differ, tiles {np.unique(bad // TILE)}, values {np.unique(got[bad])}"


def test_two_user_streams_pipeline_at_once(fresh_world, torch_cuda):
    """Two user streams on one descriptor, each with its own second stream and second scratch set: four rounds without any
    synchronisation give the serial masks."""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=(0.0, 0.02))
    Bb = 65536 + 33
    qb = sample_q(c.chain, Bb, seed=12)
    qbt = torch.from_numpy(qb).cuda()
    ref_b = {thr: c.orc.validity(qb, thr, nthreads=8) for thr in (0.0, 0.02)}
    for thr in ref_b:
        assert_tiles_mixed(ref_b[thr], ("seed 12", thr))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    with debug_option("pipe_tile", TILE):
        for rep in range(4):
            thr_a, thr_b = (0.0, 0.02) if rep % 2 == 0 else (0.02, 0.0)
            with torch.cuda.stream(s1):
                va = c.dev.validity(c.qt, thr_a)
                assert c.dev.last_tiling() == tiling(BMAX)
            with torch.cuda.stream(s2):
                wb = c.dev.validity(qbt, thr_b, packed=True)
                assert c.dev.last_tiling() == tiling(Bb)
            outs.append((thr_a, va, thr_b, wb))
        torch.cuda.synchronize()
    for rep, (thr_a, va, thr_b, wb) in enumerate(outs):
        assert np.array_equal(va.cpu().numpy(), c.ref[thr_a]), (rep, "stream 1")
        assert np.array_equal(wb.cpu().numpy(), words_of(ref_b[thr_b])), (rep, "stream 2")


def test_undersized_queues_on_both_streams(fresh_world, torch_cuda):
    """A queue budget of a few KB per scratch set: nearly every block of every tile overflows, marks itself, and is re-decided
    by k_validity_redo -- on the caller's stream and on the library's."""
    c = Case(torch_cuda, "c3", thresholds=(0.0, 0.02))
    with debug_option("pipe_tile", TILE):
        for budget in (1 << 12, 1 << 17, 1 << 21):
            with debug_option("queue_budget", budget):
                for thr in (0.0, 0.02):
                    for B in (32769, BMAX):
                        c.check(B, thr, f"budget {budget} thr={thr} B={B}", expect=tiling(B))
                        c.check(B, thr, f"budget {budget} thr={thr} B={B}", packed=True, expect=tiling(B))
        c.check(BMAX, 0.02, "back at the default budget", expect=tiling(BMAX))


BIG = 4 * 65536 + 17                            # one tile of 4097 blocks: 4 * 4097 / 256 = 64 workgroups per sub-queue before the cap


@pytest.mark.parametrize("parts", [1, 2, 64])
def test_ticketed_narrowphase_chunks(fresh_world, parts, torch_cuda):
    """narrow_parts_max caps the workgroups per sub-queue at clamp(4 * blocks / 256, 4, cap); a workgroup starts with the chunk of
    its own number and draws every further 64-item chunk from the sub-queue's ticket.  c3 at 0.02: 121 pairs and many survivors
    per row.  What decides whether the ticket is drawn is the size of ONE tile: about 256 rows feed a sub-queue of a 16 384-row
    tile, which seldom fills a second chunk, so the pipelined and the 20 000-row calls pin the launch geometry only.  The single
    tiles of 81 937 rows (1281 blocks) and of 262 161 rows (4097 blocks) hold several to dozens of chunks per sub-queue: at a
    cap of 1 or 2 nearly all of them are ticketed, and a cap of 64 launches 20 and 64 workgroups per sub-queue where the
    default cap of 16 launches 16."""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=(0.02,))
    assert c.sm.n_pairs == 121
    qb = sample_q(c.chain, BIG, seed=13)
    ref_b = c.orc.validity(qb, 0.02, nthreads=8)
    assert_tiles_mixed(ref_b, "seed 13")
    qbt = torch.from_numpy(qb).cuda()
    with debug_option("narrow_parts_max", parts):
        c.check(64, 0.02, f"parts {parts}: 64 rows")                       # four blocks or fewer: one workgroup per sub-queue anyway
        c.check(20000, 0.02, f"parts {parts}: unpipelined", expect=tiling(20000, on=False))
        c.check(20000, 0.02, f"parts {parts}: unpipelined", packed=True, expect=tiling(20000, on=False))
        c.check(BMAX, 0.02, f"parts {parts}: one tile of {BMAX} rows", expect=tiling(BMAX, on=False))
        c.check(BMAX, 0.02, f"parts {parts}: one tile of {BMAX} rows", packed=True, expect=tiling(BMAX, on=False))
        got = c.dev.validity(qbt, 0.02).cpu().numpy()
        assert c.dev.last_tiling() == tiling(BIG, on=False)
        bad = np.nonzero(got != ref_b)[0]
        assert bad.size == 0, f"parts {parts}: one tile of {BIG} rows: {bad.size} rows differ from the oracle, first at {bad[:8]}"
        words = c.dev.validity(qbt, 0.02, packed=True).cpu().numpy()
        assert np.array_equal(words, words_of(ref_b)), f"parts {parts}: one tile of {BIG} rows, words"
        with debug_option("pipe_tile", TILE):
            c.check(20000, 0.02, f"parts {parts}: below the switch", expect=tiling(20000))
            c.check(BMAX, 0.02, f"parts {parts}: pipelined", expect=tiling(BMAX))
            c.check(BMAX, 0.02, f"parts {parts}: pipelined", packed=True, expect=tiling(BMAX))
        with debug_option("pipe_tile", 2 * TILE):
            c.check(BMAX, 0.02, f"parts {parts}: pipelined, three tiles", expect=tiling(BMAX, 2 * TILE))
        c.check(64, 0.02, f"parts {parts}: 64 rows again", packed=True)


def test_movable_world_between_pipelined_calls(fresh_world, torch_cuda):
    """Obstacle moves (stream-ordered, no synchronisation) between pipelined checks: both scratch sets prepare their tables
    again after each move; a bad pose forces every row of every tile; the next good update clears it."""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=(0.0,), movable_world=True)
    assert c.dev.movable
    sets, _ = pose_sets(c.sm, 42)
    moves = [sets[1], sets[3]]
    bad = sets[1].copy()
    bad[2, 7] = np.nan
    refs = [c.ref[0.0]] + [Oracle(dataclasses.replace(c.sm, wshape_pose=P)).validity(c.q, 0.0, nthreads=8) for P in moves + [sets[5]]]
    for r in refs:
        assert_tiles_mixed(r, "moved scene")
    assert (refs[0] != refs[1]).sum() > 100 and (refs[1] != refs[2]).sum() > 100, "a move that changes nothing proves nothing"
    outs = []
    second = torch.from_numpy(moves[1]).cuda()
    torch.cuda.synchronize()
    with debug_option("pipe_tile", TILE):
        outs.append(c.dev.validity(c.qt, 0.0))
        outs.append(c.dev.validity(c.qt, 0.0, packed=True))                 # cached tables on both streams
        c.dev.set_world_poses(moves[0], stream_ordered=True)                # through the descriptor's pinned staging buffer
        outs.append(c.dev.validity(c.qt, 0.0))
        outs.append(c.dev.validity(c.qt, 0.0, packed=True))
        c.dev.set_world_poses(second)                                       # poses that are on the device already
        outs.append(c.dev.validity(c.qt, 0.0))
        outs.append(c.dev.validity(c.qt, 0.0, packed=True))
        c.dev.set_world_poses(bad, stream_ordered=True)
        outs.append(c.dev.validity(c.qt, 0.0))
        outs.append(c.dev.validity(c.qt, 0.0, packed=True))
        c.dev.set_world_poses(sets[5], stream_ordered=True)
        outs.append(c.dev.validity(c.qt, 0.0))
        outs.append(c.dev.validity(c.qt, 0.0, packed=True))
        assert c.dev.last_tiling() == tiling(BMAX)
        torch.cuda.synchronize()
    assert c.dev.world_status() == 0
    everything = np.ones(BMAX, dtype=bool)
    for k, want in enumerate((refs[0], refs[1], refs[2], everything, refs[3])):
        got = outs[2 * k].cpu().numpy()
        bad_rows = np.nonzero(got != want)[0]
        assert bad_rows.size == 0, f"step {k}: {bad_rows.size} rows differ, tiles {np.unique(bad_rows // TILE)}"
        assert np.array_equal(outs[2 * k + 1].cpu().numpy(), words_of(want)), f"step {k}: words"


def test_capture_after_a_pipelined_call(fresh_world, torch_cuda):
    """include/nbk.h: run the call once outside the capture, and captured afterwards it is a self-contained graph node.  The one
    call outside is a pipelined one here (three tiles); the captured call runs the same three tiles on the caller's stream.  (The
    diagnostic reports the host's choice; that the graph holds no work of the second stream shows in the replays, which run
    between pipelined direct calls that use that stream, as in test_graph_replays_interleaved_with_direct_calls.)"""
    torch = torch_cuda
    c = Case(torch, "c3", thresholds=())
    B, Bs = 3 * TILE, 2 * TILE + 1
    q = torch.from_numpy(sample_q(c.chain, B, seed=31)).cuda()
    qs = torch.from_numpy(sample_q(c.chain, Bs, seed=32)).cuda()
    words = torch.zeros((B // 64,), dtype=torch.int64, device="cuda")
    words_s = torch.zeros(((Bs + 63) // 64,), dtype=torch.int64, device="cuda")
    def reference(qq, thr):
        r = c.orc.validity(qq.cpu().numpy(), thr, nthreads=8)
        assert_tiles_mixed(r, thr)
        return words_of(r)
    ref = {thr: reference(q, thr) for thr in (0.0, 0.01)}
    ref_s = {thr: reference(qs, thr) for thr in (0.0, 0.01)}
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other.wait_stream(torch.cuda.current_stream())

    def direct(qq, n, thr, out, want, what):
        out.zero_()
        assert c.raw(qq, n, thr, out, None, stream=side) == 0, what
        assert c.dev.last_tiling() == tiling(n), what
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), what
    with debug_option("pipe_tile", TILE):
        with torch.cuda.stream(other):                                      # a stream without scratch: still refused
            g0 = torch.cuda.CUDAGraph()
            g0.capture_begin()
            assert c.raw(q, B, 0.01, words, None, stream=other) == -4
            g0.capture_end()
        with torch.cuda.stream(side):
            direct(q, B, 0.01, words, ref[0.01], "the call outside the capture")
            g1 = torch.cuda.CUDAGraph()
            g1.capture_begin()
            rc = c.raw(q, B, 0.01, words, None, stream=side)
            g1.capture_end()
            assert rc == 0, f"capture after a pipelined call on the same stream: status {rc} ({_lib.STATUS.get(rc)})"
            assert c.dev.last_tiling() == (3, TILE, 0)                      # the direct call's tiles, all on the caller's stream
            for seed in (41, 42):                                           # replays on new inputs
                q.copy_(torch.from_numpy(sample_q(c.chain, B, seed=seed)).cuda())
                want = reference(q, 0.01)
                words.zero_()
                g1.replay()
                side.synchronize()
                assert np.array_equal(words.cpu().numpy(), want), f"replay on seed {seed}"
            q.copy_(torch.from_numpy(sample_q(c.chain, B, seed=31)).cuda())
            for round_ in range(2):
                direct(q, B, 0.01, words, ref[0.01], "direct")
                direct(q, B, 0.0, words, ref[0.0], "direct at another threshold")
                words.zero_()
                g1.replay()
                side.synchronize()
                assert np.array_equal(words.cpu().numpy(), ref[0.01]), "replay between direct calls"
                direct(qs, Bs, 0.0, words_s, ref_s[0.0], "a smaller direct call after the replay")
                direct(qs, Bs, 0.01, words_s, ref_s[0.01], "a direct call at the graph's threshold")
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("mode", ["connect", "steer"])
def test_pipelined_edge_batches(fresh_world, mode, torch_cuda):
    """1500 edges at resolution 0.02 and max_distance 1.0: a flat batch of 78 016 slots, five tiles.  steer() stops at
    max_distance, so its samples fit and every call has that tiling; connect() walks the whole edge, the first call overflows
    (those edges are walked one wave each) and later calls size the batch from the count the device reported."""
    c = Case(torch_cuda, "c2", thresholds=())
    E, SLOTS = 1500, 78016
    s, g = c.q[:E], c.q[E:2 * E]
    first = True
    for thr in (0.0, 0.02):
        okr, endr, nsr = c.orc.edge_validity(s, g, 0.02, 1.0, mode=mode, threshold=thr, nthreads=8)
        total = int(nsr.sum())
        assert 0 < okr.sum() < E and (total <= SLOTS - 16) == (mode == "steer") and (total > 4 * SLOTS) == (mode == "connect")
        with debug_option("pipe_tile", TILE):
            for rep in range(2):
                ok, end, ns = c.dev.edge_validity(s, g, 0.02, 1.0, mode=mode, threshold=thr)
                tiles, rows, piped = c.dev.last_tiling()
                if first or mode == "steer":
                    assert (tiles, rows, piped) == (5, TILE, 1), (mode, thr, rep)
                else:
                    assert (rows, piped) == (TILE, 1) and tiles * TILE >= total, (mode, thr, rep, tiles)
                first = False
                assert np.array_equal(ok, okr) and np.array_equal(ns, nsr), (mode, thr, rep)
                assert_bitwise(end, endr, f"{mode} ends")
        ok, end, ns = c.dev.edge_validity(s, g, 0.02, 1.0, mode=mode, threshold=thr)
        tiles, rows, piped = c.dev.last_tiling()
        assert (tiles, piped) == (1, 0) and (rows == SLOTS if mode == "steer" else rows >= total), (mode, thr, rows)
        assert np.array_equal(ok, okr) and np.array_equal(ns, nsr), (mode, thr, "unpipelined")
        assert_bitwise(end, endr, f"{mode} ends, unpipelined")


def test_pipelined_edge_batches_beyond_the_scratch_capacity(fresh_world, torch_cuda):
    """The over-long edges of test_edge_batches_beyond_the_scratch_capacity, 1300 of them: 35 136 slots pipeline as three tiles
    and overflow; the next call sizes its scratch from what the device reported, so the tile count changes between calls."""
    c = Case(torch_cuda, "c2", thresholds=())
    E = 1300
    rng = np.random.default_rng(3)
    base = sample_q(c.chain, 1, seed=9)[0] * 0.2
    s_ = base + rng.uniform(-0.3, 0.3, (E, 7))
    g_ = s_ + rng.uniform(-1.0, 1.0, (E, 7)) * rng.uniform(0.1, 3.0, (E, 1))
    okr, endr, nsr = c.orc.edge_validity(s_, g_, 0.01, 0.25, mode="connect", nthreads=8)
    assert nsr.sum() > 3 * E * 27 and 0 < okr.sum() < E
    seen = []
    with debug_option("pipe_tile", TILE):
        for rep in range(3):
            ok, end, ns = c.dev.edge_validity(s_, g_, 0.01, 0.25, mode="connect")
            seen.append(c.dev.last_tiling())
            assert np.array_equal(ok, okr) and np.array_equal(ns, nsr), rep
            assert_bitwise(end, endr, "overflow edge ends")
        assert seen[0] == (3, TILE, 1), seen
        assert seen[1][1:] == (TILE, 1) and seen[1][0] * TILE >= int(nsr.sum()) > seen[0][0] * TILE, seen      # grown to what was needed
        assert seen[2] == seen[1], seen
        ok, end, ns = c.dev.edge_validity(s_, g_, 0.01, 0.25, mode="steer")
        assert c.dev.last_tiling() == seen[1]
    okr, endr, nsr = c.orc.edge_validity(s_, g_, 0.01, 0.25, mode="steer", nthreads=8)
    assert np.array_equal(ok, okr) and np.array_equal(ns, nsr) and nsr.max() <= 27
    assert_bitwise(end, endr, "steer ends")
