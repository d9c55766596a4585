"""What cimrgp_potrf reports, and leaves behind, when a pivot fails -- on every schedule path.

The failing pivot is exact by construction (potrf_failure_numpy: an injected diagonal entry; test_potrf_failure_host.py
confirms every expectation with dpotrf and spotrf on the CPU).  For a failure at order j, with c0 / k0 the first column
of the 64-column block / 256-column panel that holds column j-1:

  (a) info == j exactly (never CIMRGP_INFO_WATCHDOG);
  (b) the columns of L left of c0 are bit for bit those of the library's factor of the un-injected matrix (the schedule
      is right-looking: they are final before the failing block is touched and never written again);
  (c) the carried rows' columns left of k0 are bit for bit those of the clean run;
  (d) the clean factor itself is checked once per (n, dtype) against LAPACK (FP64: 1e-10 relative to max |L|; FP32: the
      backward-error bar 64 sqrt(n) eps32 of test_potrf_f32_lookahead_backward_error).

Then: the look-ahead context is untouched by a failed run, no path forgets to clear a stale info word, every block of a
batch owns its word, and a failure inside the staged pipeline stays in its block.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import oracle
import potrf_failure_numpy as pf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": "float64", "f32": "float32"}
WATCHDOG = 0x7fffffff
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _tdt(dt):
    return getattr(torch, TDT[dt])


def _case_id(case):
    n, m, inj = case
    return "n%d-m%d-%s" % (n, m, "+".join("j%d(%g)" % (j, v) for j, v in inj))


def _gram(dev, n, tdt, seed=None, out=None):
    """The clean base matrix on the device (lower triangle)."""
    xd = dev.to_device(pf.points(n, seed), tdt, "cuda")
    return dev.rbf_gram(xd, pf.ELL, pf.SF2, pf.NOISE, lower_only=True, out=out)


def _rows(dev, n, m, tdt):
    bbuf = dev.alloc_matrix(m, n, tdt, "cuda")
    bbuf[:m, :n] = torch.from_numpy(pf.carried_rows(n, m)).to("cuda", tdt)
    return bbuf


def _factor(dev, n, tdt, m, injections=(), ws=None, info=None):
    """Gram matrix on the device, the injected diagonal entries, the factorisation (with m carried rows).
    Returns (kbuf, bbuf or None, ws, info)."""
    kbuf = _gram(dev, n, tdt)
    for j, value in injections:
        kbuf[j - 1, j - 1] = value
    if m:
        bbuf = _rows(dev, n, m, tdt)
        ws, info = dev.potrf_rows(kbuf, n, bbuf, m, ws=ws, info=info)
    else:
        bbuf = None
        ws, info = dev.potrf(kbuf, n, ws=ws, info=info)
    return kbuf, bbuf, ws, info


def _lower(kbuf, n):
    return torch.tril(kbuf[:n, :n])


_LAPACK = {}     # n -> LAPACK's FP64 factor of the clean matrix, on the device (computed once per module)
_GOOD = {}       # (n, dt, m) -> (lower triangle of the library's clean factor, its carried rows or None)


def _lapack_factor(n):
    if n not in _LAPACK:
        lref, iref = oracle.potrf_lower(pf.base_gram(pf.points(n)))
        assert iref == 0
        _LAPACK[n] = torch.from_numpy(lref).cuda()
    return _LAPACK[n]


def _check_clean_factor(dev, n, dt, lgood, bgood, m):
    """(d): the library's clean factor against the reference."""
    if dt == "f64":
        lref = _lapack_factor(n)
        err = float((lgood - lref).abs().max() / lref.abs().max())
        print("clean factor n=%d f64 m=%d: max |L - L_lapack| / max |L| = %.3e (bar 1e-10)" % (n, m, err))
        assert err < 1e-10, err
        if m:
            want = sla.solve_triangular(lref.cpu().numpy(), pf.carried_rows(n, m).T, lower=True).T        # B L^-T
            got = bgood[:m, :n].cpu().numpy()
            errb = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            print("clean rows   n=%d f64 m=%d: %.3e (bar 1e-9)" % (n, m, errb))
            assert errb < 1e-9, errb                 # the bar of test_potrf_lookahead_path_matches_lapack
    else:
        k64 = _lower(_gram(dev, n, torch.float32), n).double()
        k64 = k64 + torch.tril(k64, -1).t()
        l64 = lgood.double()
        resid = float(torch.linalg.norm(l64 @ l64.t() - k64) / torch.linalg.norm(k64))
        print("clean factor n=%d f32 m=%d: |L L^T - K|_F / |K|_F = %.3e (bar %.3e)" % (n, m, resid, 64 * np.sqrt(n) * EPS32))
        assert resid < 64 * np.sqrt(n) * EPS32, resid


def _good(dev, n, dt, m):
    """The library's factor (and carried rows) of the un-injected matrix: once per (n, dtype, m), checked (d)."""
    key = (n, dt, m)
    if key not in _GOOD:
        kbuf, bbuf, _, info = _factor(dev, n, _tdt(dt), m)
        assert int(info.item()) == 0
        lgood = _lower(kbuf, n).clone()
        _check_clean_factor(dev, n, dt, lgood, bbuf, m)
        _GOOD[key] = (lgood, None if bbuf is None else bbuf[:m, :n].clone())
    return _GOOD[key]


# ------------------------------------------------------------------------------------------------ single matrices ----

SINGLE = [c for c in pf.single_cases() if c[0] != pf.PAIRED[0]]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", SINGLE, ids=_case_id)
def test_failing_pivot_is_reported_exactly_and_the_columns_left_of_it_are_final(dev, dt, case):
    """One queue (n = 700, 641: fused_sweep, nine-wave k_diag64 / k_link, ragged last block, carried rows in the chain's
    launches) and look-ahead (n = 6144: panel 0 nine-wave, look-ahead panels four-wave k_diag64q / k_linkq -- gated in
    FP64 without rows, ungated otherwise --, the one-queue tail, carried rows on their own queues): (a), (b), (c)."""
    n, m, inj = case
    lgood, bgood = _good(dev, n, dt, m)
    kbuf, bbuf, _, info = _factor(dev, n, _tdt(dt), m, inj)
    j = pf.expected_info(inj)
    got = int(info.item())
    assert got != WATCHDOG
    assert got == j                                                           # (a)
    c0, k0 = pf.block_start(j), pf.panel_start(j)
    assert torch.equal(_lower(kbuf, n)[:, :c0], lgood[:, :c0])                # (b)
    if m:
        assert torch.equal(bbuf[:m, :k0], bgood[:, :k0])                      # (c)
    with pytest.raises(np.linalg.LinAlgError):
        dev.raise_if_not_pd(info)


def _clean_bad_clean(dev, n, dt, m, j):
    """Clean, injected, clean on one stream with one workspace and one info word: the third run is the first."""
    tdt = _tdt(dt)
    k1, b1, ws, info = _factor(dev, n, tdt, m)
    assert int(info.item()) == 0
    _, _, _, info = _factor(dev, n, tdt, m, ((j, -1.0),), ws=ws, info=info)
    assert int(info.item()) == j
    k3, b3, _, info = _factor(dev, n, tdt, m, ws=ws, info=info)
    assert int(info.item()) == 0
    assert torch.equal(_lower(k3, n), _lower(k1, n))
    if m:
        assert torch.equal(b3[:m, :n], b1[:m, :n])
    return k1, b1


@pytest.mark.parametrize("j", [700, 4000])
@pytest.mark.parametrize("m", pf.LOOKAHEAD_M)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_context_survives_a_failed_factorisation(dev, dt, m, j):
    """A run full of NaNs goes through the device-side gate, the context's flag words and its last_done event
    (j = 700: look-ahead phase, j = 4000: tail).  The next factorisation on the same context must not notice."""
    n = pf.LOOKAHEAD_N
    k1, b1 = _clean_bad_clean(dev, n, dt, m, j)
    lgood, bgood = _good(dev, n, dt, m)
    assert torch.equal(_lower(k1, n), lgood)
    if m:
        assert torch.equal(b1[:m, :n], bgood)


def test_failure_beside_paired_far_updates(dev):
    """n = 10240 > far_pair_above: the first look-ahead steps update the far part once per two panels (K = 512).
    (a) and the reuse check only (no CPU factor of this size)."""
    n, j = pf.PAIRED
    _clean_bad_clean(dev, n, "f64", 0, j)


# -------------------------------------------------------------------------------------------- a stale info word ----

@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [700, pf.LOOKAHEAD_N])
def test_potrf_clears_a_stale_info_word(dev, dt, n):
    """The kernels only write over 0 (atomicCAS): a path that forgot its memset would report success forever after --
    or a stale failure.  One queue and look-ahead."""
    info = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    _, _, _, got = _factor(dev, n, _tdt(dt), 0, info=info)
    assert got.data_ptr() == info.data_ptr()
    assert int(info.item()) == 0


# ------------------------------------------------------------------------------------------------------ batched ----

def _batched_run(dev, n, batch, tdt, bad):
    ld = dev.padded_ld(n)
    karena = torch.empty((batch, n, ld), dtype=tdt, device="cuda")
    ws_bytes = (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16
    ws_arena = torch.empty((batch, max(ws_bytes, 16)), dtype=torch.uint8, device="cuda")
    info = torch.full((batch,), 12345, dtype=torch.int32, device="cuda")          # stale words: every one is cleared
    for i in range(batch):
        _gram(dev, n, tdt, seed=pf.batch_seed(n, i), out=karena[i])
        if i in bad:
            karena[i, bad[i] - 1, bad[i] - 1] = -1.0
    dev.potrf_rows_batched(karena, n, ld, ws_arena, info)
    return karena, info.cpu().tolist()


@pytest.mark.parametrize("n,batch,bad,dt", [c + ("f64",) for c in pf.BATCHED] + [pf.BATCHED[0] + ("f32",)],
                         ids=lambda v: str(v) if not isinstance(v, dict) else "bad" + "_".join("%d@%d" % (j, b) for b, j in v.items()))
def test_batched_every_block_reports_its_own_word(dev, n, batch, bad, dt):
    """3 x 320: fused_sweep with riders; 25 x 1024: two halves of 12 and 13 on two queues (the second half's words
    start at info + 12); 7 x 3584: panel_sweep on one queue.  Four-wave kernels throughout, info += blockIdx.y."""
    tdt = _tdt(dt)
    clean, info_clean = _batched_run(dev, n, batch, tdt, {})
    assert info_clean == [0] * batch
    got, info_bad = _batched_run(dev, n, batch, tdt, bad)
    assert info_bad == [bad.get(i, 0) for i in range(batch)]
    for i in range(batch):
        c0 = pf.block_start(bad[i]) if i in bad else n
        assert torch.equal(torch.tril(got[i][:, :n])[:, :c0], torch.tril(clean[i][:, :n])[:, :c0]), i
    i = next(b for b in range(batch) if b not in bad)
    lgot = torch.tril(got[i][:, :n]).double()
    if dt == "f64":
        lref, iref = oracle.potrf_lower(pf.base_gram(pf.points(n, pf.batch_seed(n, i))))
        assert iref == 0
        lref = torch.from_numpy(lref).cuda()
        assert float((lgot - lref).abs().max() / lref.abs().max()) < 1e-10
    else:
        k64 = torch.tril(_gram(dev, n, tdt, seed=pf.batch_seed(n, i))[:n, :n]).double()
        k64 = k64 + torch.tril(k64, -1).t()
        resid = float(torch.linalg.norm(lgot @ lgot.t() - k64) / torch.linalg.norm(k64))
        assert resid < 64 * np.sqrt(n) * EPS32, resid


# ---------------------------------------------------------------------------------------------- staged pipeline ----

@pytest.mark.parametrize("front", [False, True])
def test_a_failure_inside_the_staged_pipeline_stays_in_its_block(dev, front):
    """cimrgp_block_posterior_staged builds its own Gram matrix, so block 1 fails through its inputs (a duplicated point,
    no noise: order 3000 on the CPU, 3000 or 3001 with the device's Gram matrix -- the rounding-level tolerance
    test_gpu_layer.py grants).  Four blocks over two rotating buffer sets, each with its own info word; with a front
    queue the info word is cleared on another queue than in the plain call.  Blocks 0, 2 and 3 are bit for bit the
    one-stream results: block 2 starts beside the failed block's NaN-filled tail, block 3 reuses its buffer set."""
    tdt = torch.float64
    n, ns, q = pf.STAGED_N, 130, 2
    nblocks, nsets, bad = 4, 2, 1
    rng = np.random.default_rng(n + 1)
    blocks = []
    for b in range(nblocks):
        x = np.sort(rng.uniform(-2.0, 2.0, size=(n, 1)), axis=0)
        y = np.stack([np.cos(3 * x[:, 0] + c + b) for c in range(q)], axis=1) + 0.1 * rng.normal(size=(n, q))
        xs = rng.uniform(-2.0, 2.0, size=(ns, 1))
        if b == bad:
            x = pf.staged_bad_points()
        blocks.append(tuple(dev.to_device(a, tdt, "cuda") for a in (x, y, xs)))
    sf2 = 1.1
    hyper = [(pf.STAGED_ELL, 0.0) if b == bad else (0.05, 0.02) for b in range(nblocks)]

    def buffers():
        return dict(kbuf=dev.alloc_matrix(n, n, tdt, "cuda"), wbuf=dev.alloc_matrix(ns + q, n, tdt, "cuda"),
                    ws=dev.potrf_workspace(n, tdt, "cuda"),
                    alpha=torch.zeros((n, q), dtype=tdt, device="cuda"), z=torch.zeros((n, q), dtype=tdt, device="cuda"),
                    scratch=torch.empty(2 * q * n, dtype=tdt, device="cuda"))
    means = [torch.zeros((ns, q), dtype=tdt, device="cuda") for _ in range(2 * nblocks)]
    vars_ = [torch.zeros(ns, dtype=tdt, device="cuda") for _ in range(2 * nblocks)]
    infos = [torch.full((1,), 12345, dtype=torch.int32, device="cuda") for _ in range(2 * nblocks)]
    bs = buffers()
    for i, (xd, yd, xsd) in enumerate(blocks):
        if i == bad:
            continue
        dev.block_posterior(xd, yd, xsd, hyper[i][0], sf2, hyper[i][1], bs["kbuf"], bs["wbuf"], bs["ws"], infos[i], bs["alpha"],
                            bs["z"], means[i], vars_[i], scratch=bs["scratch"])
    torch.cuda.synchronize()
    assert [int(infos[i].item()) for i in range(nblocks) if i != bad] == [0, 0, 0]
    cur = torch.cuda.current_stream()
    sq = dev.solve_queue(cur)
    fq = dev.front_queue(cur) if front else cur
    sets = [buffers() for _ in range(nsets)]
    torch.cuda.synchronize()
    for i, (xd, yd, xsd) in enumerate(blocks):
        b = sets[i % nsets]
        dev.block_posterior(xd, yd, xsd, hyper[i][0], sf2, hyper[i][1], b["kbuf"], b["wbuf"], b["ws"], infos[nblocks + i],
                            b["alpha"], b["z"], means[nblocks + i], vars_[nblocks + i], scratch=b["scratch"], streams=(fq, cur, sq))
    torch.cuda.synchronize()
    got = [int(infos[nblocks + i].item()) for i in range(nblocks)]
    assert got[bad] in (pf.STAGED_J, pf.STAGED_J + 1), got
    assert [g for i, g in enumerate(got) if i != bad] == [0, 0, 0], got
    for i in range(nblocks):
        if i != bad:
            assert torch.equal(means[i], means[nblocks + i]) and torch.equal(vars_[i], vars_[nblocks + i]), i
