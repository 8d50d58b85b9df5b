"""Gradient clipping and weight decay inside the optimiser on host tensors
(DESIGN.md "Device learner step"): mbots_policy_adam_clip against its float32
restatement bit for bit, its squared norms against math.fsum, one step against
float64 within the derived bound and against clip_grad_norm_ + AdamW as a
sanity check; PolicyAdam(max_grad_norm=, weight_decay=).  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import policy_adam_ref as ar
import policy_adam_util as au
import policy_seq_loss_ref as sr
import policy_seq_loss_util as u

WD = 0.01


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def trace():
    import madrona_bots as mb
    return u.run_clip(mb, "cpu", WD, u.MAX_NORM)


@pytest.fixture(scope="module")
def restated():
    """The restatement's snapshots after each step, and the squared norms of step 0."""
    P = [a.copy() for a in u.clip_params()]
    M, V = [np.zeros_like(a) for a in P], [np.zeros_like(a) for a in P]
    state = ar.adam_state(u.CLIP_GROUPS)
    rows = u.clip_rows().tolist()
    out = []
    for k in range(u.CLIP_STEPS):
        G = u.clip_gradients(k)
        tensors = [(P[i], G[i], M[i], V[i], g) for i, g in enumerate(u.clip_groups())]
        with np.errstate(over="ignore", invalid="ignore"):
            norms = sr.adam_clip_f32(tensors, state, rows, weight_decay=WD, max_norm=u.MAX_NORM, **u.CLIP_HYPER)
        out.append(([a.copy() for a in P], [a.copy() for a in M], [a.copy() for a in V], list(state), norms))
    return out


def test_case_covers_the_lengths_and_groups(trace):
    sizes, groups = u.clip_sizes(), u.clip_groups()
    assert len(sizes) == 70 > 64 and set(sizes) == {1, 3, 1023, 1024, 1025, 4100}
    assert all({n for n, g in zip(sizes, groups) if g == k} == set(sizes) for k in range(u.CLIP_GROUPS))
    assert sizes[u.UNALIGNED] == 1025 and groups[u.UNALIGNED] == u.CLIPPED
    norm = trace[0][4]
    assert norm[u.CLIPPED] > u.MAX_NORM > norm[u.UNCLIPPED] > 0 and norm[u.IDLE] > 0 and np.isinf(norm[u.INF])


def test_three_steps_equal_the_float32_restatement(trace, restated):
    """param, m, v, state and grad_norm after each step: the clipped group, the
    one below the bound, the idle one and the one whose first gradient holds an
    inf (untouched at step 0, then two steps behind in nothing but its count)."""
    for k, (got, want) in enumerate(zip(trace, restated)):
        for name, a, b in zip(("param", "m", "v"), got[:3], want[:3]):
            for i in range(u.CLIP_TENSORS):
                assert np.array_equal(bits(a[i]), bits(b[i])), f"step {k}, {name} of tensor {i}"
        for g, (tt, b1t, b2t) in enumerate(want[3]):
            assert got[3][g].tolist() == [tt, int(np.float32(b1t).view(np.int32)), int(np.float32(b2t).view(np.int32))]
        assert np.array_equal(bits(got[4]), bits(want[4])), f"step {k}: grad_norm {got[4]} != {want[4]}"
    assert trace[-1][3][:, 0].tolist() == [3, 3, 0, 2]


def test_idle_and_inf_groups_are_left_untouched(trace):
    P0 = u.clip_params()
    params, m, v, state, norm = trace[0]
    for i, g in enumerate(u.clip_groups()):
        if g in (u.IDLE, u.INF):
            assert np.array_equal(bits(params[i]), bits(P0[i])) and not bits(m[i]).any() and not bits(v[i]).any()
        else:
            assert m[i].any() and not np.array_equal(params[i], P0[i])
    assert state[u.IDLE].tolist() == state[u.INF].tolist() == [0, 0x3F800000, 0x3F800000]
    assert norm[u.INF] == np.inf and np.isfinite(norm[u.IDLE])


def test_unclipped_group_equals_the_plain_step():
    """Without weight decay a group below the bound (coef == 1) ends with the
    bits of mbots_policy_adam; max_norm = inf, <= 0 and NaN turn clipping off
    for every group."""
    import madrona_bots as mb
    rows = u.clip_rows()

    def run(step):
        opt = u.RawAdam(mb, u.clip_params(), u.clip_groups(), u.CLIP_GROUPS, "cpu", unaligned=(u.UNALIGNED,))
        G = u.clip_gradients(0)
        G = [np.where(np.isinf(g), np.float32(1.0), g) for g in G]
        opt.set_gradients(G)
        step(opt)
        return opt.snapshot()
    plain = run(lambda o: o.step_plain(rows, **u.CLIP_HYPER))
    clipped = run(lambda o: o.step_clip(rows, 0.0, u.MAX_NORM, **u.CLIP_HYPER))
    same = lambda a, b, i: all(np.array_equal(bits(a[k][i]), bits(b[k][i])) for k in range(3))
    for i, g in enumerate(u.clip_groups()):
        assert same(plain, clipped, i) == (g in (u.UNCLIPPED, u.IDLE)), i         # (INF's finite stand-in is clipped)
    assert np.array_equal(plain[3], clipped[3])
    for off in (float("inf"), 0.0, -1.0, float("nan")):
        got = run(lambda o: o.step_clip(rows, 0.0, off, **u.CLIP_HYPER))
        assert all(same(plain, got, i) for i in range(u.CLIP_TENSORS)) and np.array_equal(plain[3], got[3])
        assert got[4][u.CLIPPED] > u.MAX_NORM                                  # the norm is still reported


def test_squared_norm_against_fsum(trace, restated):
    """N^2 of the restatement (whose grad_norm the library matches to the bit)
    against math.fsum of the exact squares: all terms are non-negative, so the
    relative error is at most (additions on the longest chain) * 2^-53 -- 3 into
    an accumulator, 8 tree levels, the tensor's chunks and the group's tensors."""
    G = u.clip_gradients(1)
    groups = u.clip_groups()
    n2 = sr.group_normsq([(None, g, None, None, k) for g, k in zip(G, groups)], u.CLIP_GROUPS)
    for k in range(u.CLIP_GROUPS):
        mine = [g for g, gk in zip(G, groups) if gk == k]
        exact = math.fsum(float(x) * float(x) for g in mine for x in g.tolist())
        chain = 3 + 8 + max(-(-g.size // 1024) for g in mine) + len(mine)
        rel = abs(n2[k] - exact) / exact
        print(f"group {k}: N^2 {n2[k]!r}, relative error {rel:.3e}, bound {chain * 2.0 ** -53:.3e}")
        assert rel <= chain * 2.0 ** -53
        assert trace[1][4][k] == np.float32(np.sqrt(n2[k]))


def test_paths_of_the_chunk_sum_agree():
    """The 16-byte and the 4-byte path, whole chunks and tails: the norm of one
    tensor does not depend on where it lies."""
    import madrona_bots as mb
    rng = np.random.default_rng(3)
    for n in (1, 3, 1023, 1024, 1025, 4100):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
        norms = []
        for unaligned in ((), (0,)):
            opt = u.RawAdam(mb, [np.zeros(n, np.float32)], [0], 1, "cpu", unaligned=unaligned)
            opt.set_gradients([g])
            opt.step_clip(None, 0.0, 1.0, **u.CLIP_HYPER)
            norms.append(opt.snapshot()[4][0])
        assert bits(norms[0]) == bits(norms[1]) == bits(np.float32(np.sqrt(sr.tensor_sq(g)))), n


def test_one_step_against_float64(trace):
    """|p'_f32 - p'_f64| <= 2 * 2^-24 (|p'| + |p1| + |lw p| + 24 A) from the common
    f32 state (DESIGN.md "Device learner step" derives it)."""
    P0, G = u.clip_params(), u.clip_gradients(0)
    groups = u.clip_groups()
    exact = [math.fsum(float(x) * float(x) for g, gk in zip(G, groups) if gk == k for x in g.tolist())
             for k in (u.CLIPPED, u.UNCLIPPED)]
    worst = 0.0
    for i, k in enumerate(groups):
        if k not in (u.CLIPPED, u.UNCLIPPED):
            continue
        z = np.zeros_like(P0[i])
        want, bound = sr.adam_clip_f64(P0[i], G[i], z, z, 0, exact[k], weight_decay=WD, max_norm=u.MAX_NORM,
                                       **u.CLIP_HYPER)
        err = np.abs(trace[0][0][i].astype(np.float64) - want)
        assert (err <= bound).all(), i
        worst = max(worst, float((err / bound).max()))
    print(f"worst error / bound: {worst:.3f}")


def test_against_torch_clip_and_adamw(trace):
    """A sanity check only: clip_grad_norm_ + torch.optim.AdamW on the clipped
    and the unclipped group, within the float64 bound above plus as much again
    for torch's own float32 arithmetic."""
    P0, G = u.clip_params(), u.clip_gradients(0)
    groups = u.clip_groups()
    for k in (u.CLIPPED, u.UNCLIPPED):
        idx = [i for i, gk in enumerate(groups) if gk == k]
        ps = [torch.from_numpy(P0[i].copy()).requires_grad_() for i in idx]
        for p, i in zip(ps, idx):
            p.grad = torch.from_numpy(G[i].copy())
        total = torch.nn.utils.clip_grad_norm_(ps, u.MAX_NORM)
        assert abs(float(total) - float(trace[0][4][k])) <= 1e-5 * float(total)
        torch.optim.AdamW(ps, weight_decay=WD, **u.CLIP_HYPER).step()
        exact = math.fsum(float(x) * float(x) for i in idx for x in G[i].tolist())
        for p, i in zip(ps, idx):
            z = np.zeros_like(P0[i])
            _, bound = sr.adam_clip_f64(P0[i], G[i], z, z, 0, exact, weight_decay=WD, max_norm=u.MAX_NORM,
                                        **u.CLIP_HYPER)
            assert (np.abs(p.detach().numpy().astype(np.float64) - trace[0][0][i]) <= 2.0 * bound).all(), i


def test_policy_adam_options():
    """PolicyAdam without options and with max_grad_norm = inf leaves bit for
    bit today's step (policy_adam_util's three steps); with options it equals
    the raw call, holds grad_norm [G] and keeps state_dict()'s keys."""
    import madrona_bots as mb

    def three_steps(**kw):
        opt = mb.PolicyAdam(au.make_groups(mb, "cpu"), **au.HYPER, **kw)
        rows = au.rows_of("cpu")
        for k in range(au.STEPS):
            au.set_gradients(opt, au.gradients(opt, k))
            opt.step(rows)
        return opt
    plain, default, inf = au.run_adam(mb, "cpu")[0], three_steps(), three_steps(max_grad_norm=float("inf"))
    assert default._ws is None and inf._ws is not None
    for other in (default, inf):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain.params, other.params))
        sd, so = plain.state_dict(), other.state_dict()
        assert sorted(sd) == sorted(so) == ["m", "state", "v"]
        assert all(torch.equal(sd[k].view(torch.int32), so[k].view(torch.int32)) for k in sd)
    assert inf.grad_norm.shape == (au.GROUPS,) and inf.grad_norm.dtype == torch.float32 and (inf.grad_norm > 0).all()

    opt = three_steps(max_grad_norm=0.5, weight_decay=WD)
    P = [p.detach().numpy().copy() for p in au.run_adam(mb, "cpu")[1]]
    M, V = [np.zeros_like(a) for a in P], [np.zeros_like(a) for a in P]
    state = ar.adam_state(au.GROUPS)
    for k in range(au.STEPS):
        G = au.gradients(opt, k)
        norms = sr.adam_clip_f32([(P[i], G[i], M[i], V[i], opt.param_group[i]) for i in range(len(P))], state,
                                 au.rows_of("cpu").tolist(), weight_decay=WD, max_norm=0.5, **au.HYPER)
    assert all(np.array_equal(bits(p.detach().numpy()), bits(a)) for p, a in zip(opt.params, P))
    assert np.array_equal(bits(opt.grad_norm.numpy()), bits(norms))
    assert any(not torch.equal(a, b) for a, b in zip(plain.params, opt.params))
    with pytest.raises(ValueError, match="max_grad_norm must be a positive number"):
        mb.PolicyAdam(au.make_groups(mb, "cpu"), max_grad_norm=0.0)
    with pytest.raises(ValueError, match="weight_decay must be a finite number"):
        mb.PolicyAdam(au.make_groups(mb, "cpu"), weight_decay=-1.0)


def test_workspace_is_checked():
    import madrona_bots as mb
    opt = u.RawAdam(mb, [np.zeros(5, np.float32), np.zeros(2049, np.float32)], [0, 1], 2, "cpu")
    assert opt.ws_bytes == (1 + 3) * 8 + 2 * 8 + 2 * 8 + 2 * 8       # chunks, tensors, then normsq, coef and live
    opt.ws_bytes -= 1
    with pytest.raises(RuntimeError, match=r"workspace of 79 bytes, 80 needed \(mbots_policy_adam_clip_workspace\)"):
        opt.step_clip(None, 0.0, 1.0, **u.CLIP_HYPER)
    need = ctypes.c_uint64()
    assert mb._lib.mbots_policy_adam_clip_workspace(opt.desc, 2, 65, ctypes.byref(need)) != 0
