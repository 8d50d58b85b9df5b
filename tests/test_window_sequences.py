"""Random call sequences with a trajectory window open and renders queued,
against the oracle: the operations of
tests/test_parity_gpu.py::run_episode_sequence with a push behind every step,
a compute / clear(keep_last) whenever the window is full, and render_worlds
calls whose images are read only later.  Every expectation comes from the
oracle (tests/window_ref.py), none from the product, and every comparison is
bitwise.  The CPU half runs anywhere; the device half crosses the push and the
queued render with the three step schedules (K1-finder, joined at 4100 worlds,
swapped at 16400), the reset pass, in-place growth, pending lazy shifts and
checkpoint loads.

Mutation checks on scratch builds (value-only errors, one per build): a
traj_slot that ignores base, a traj_end that reads table t's marks and a
rasteriser in which the highest slot wins each fail all eight CPU-mode seeds;
on the device a band cull of reach 0.5 fails all six K1-finder seeds, and a
push ordered after what precedes the step's export instead of after the
export fails seed 100 at 16400 worlds (69560 of 524800 links of one table
stale) -- a race the export can win, as it did in the other three sequences
of the large world counts."""
import numpy as np
import pytest
import torch

import pyoracle
import window_ref as wr
from simpair import COLUMNS, bits, compare, gpu_column

HORIZON = 6
PARAMS = ((0.99, 0.95, -1.0), (1.0, 1.0, 0.0))
SCALES, SCALE_P = (1, 2, 4, 8), (0.3, 0.3, 0.3, 0.1)
RENDER_KEYS = ("rgb", "cls", "slot")

# Chosen by running the CPU mode (scripts/fuzz_calls.py --window --cpu): every
# seed meets run_window_sequence's non-vacuity conditions at its world count.
# The seeds of the large world counts are ones whose sequences hold few steps
# (14 to 16 of the 64 operations), for the oracle's sake.
CPU_SEEDS = [1, 2, 3, 4, 5, 6, 7, 8]      # 20 + seed worlds
GPU_SEEDS = [1, 2, 3, 4, 5, 6]            # 20 + seed worlds: the K1-finder mode
GPU_SEEDS_JOINED = [9, 13]                # 4100 worlds
GPU_SEEDS_SWAPPED = [100, 118]            # 16400 worlds
GPU_SEEDS_STREAM = [7, 8]                 # 20 + seed worlds, on a side stream


def run_window_sequence(seed, W=None, exec_mode="hip"):
    """64 random operations on an armed manager of 128 slots with a window of
    6 tables, and on an oracle of 1024 slots taking the same calls.

    Before every step both sides get row + 1 stamped into column 0 of the
    current HiddenState (after the last action or hidden write), so the oracle's
    column after the step names each row's previous row: the reference's link.
    The values of the table the step will produce are uploaded before the step
    (their count is the oracle's, which steps first), so step() and push()
    follow each other with no host synchronisation in between.  When the window
    is full before a step it is computed -- sometimes twice, with other
    parameters, before anything is read --, checked and cleared with
    keep_last; it is also checked before a load or a set_world_state empties it
    and at the end.  Renders are compared at the next full comparison, after
    whatever steps, resets or growths followed them.

    max_rows: twice the oracle's row count when the window is opened, which the
    oracle's peak row count stays under (asserted at every push).

    Returns what the sequence did; the non-vacuity conditions asserted at the
    end are computed from the reference alone."""
    from reset_util import episode_errors
    from test_parity_gpu import _obs_rows_oracle
    import madrona_bots as mb
    rng = np.random.default_rng(seed)
    caps = np.random.default_rng(seed + 1000)
    W = W or 20 + seed
    fixd = bool(seed % 2)
    classes = [c for c in mb.CAPACITY_CLASSES if c <= 1024]
    pal = np.asarray(mb.RENDER_PALETTE)
    mgr = mb.SimManager(0, W, 69, 32, fix_depth_alias=fixd, exec_mode=exec_mode)
    orc = pyoracle.OracleSim(W, 69, 32, cap=1024, num_threads=16 if W >= 4096 else 8)
    flags = mgr.reset_tensor().to_torch()   # (arms the manager)
    oflags = orc.reset_flags()
    special = [w for w in (0, W - 1, 1023, 1024) if 0 <= w < W]
    quiet = set()       # worlds whose scene was set since their last step
    rec = wr.WindowRecorder(orc, seed)
    info = {"steps": 0, "window_checks": 0, "chained_clears": 0, "checks_after_chained_clear": 0, "births": 0,
            "deaths": 0, "alive": 0, "reset_cuts": 0, "renders": 0, "renders_after_later_step": 0, "restarts": 0,
            "grown": 0, "peak_population": 0, "peak_rows": 0}
    pending = []        # queued renders: (outputs, expected, steps when issued)
    chained = False     # the window now open began with a clear(keep_last)
    t = 0

    def upload(v, rows):
        """v padded to `rows` entries on the manager's device, without a wait
        (a buffer of max_rows entries spares push() its row-count read)."""
        buf = torch.zeros(rows, dtype=torch.float32)
        buf[:v.numel()] = v
        if exec_mode != "hip":
            return buf
        return buf.pin_memory().to(mgr.device, non_blocking=True)

    def open_window():
        rows = 2 * orc.num_agents()
        win = mgr.trajectory_window(HORIZON, rows)
        restart(win)
        return win

    def restart(win):
        """The emptied (or new) window's first table: the current one."""
        nonlocal chained
        assert win.num_tables == 0
        rec.restart()
        chained = False
        assert orc.num_agents() <= win.max_rows
        win.push(upload(rec.values(t), win.max_rows))
        rec.table(t, stepped=False)
        info["restarts"] += 1

    def window_check(where, clear):
        nonlocal chained
        if len(rec) < 2:
            return
        params = PARAMS[0]
        out = win.compute(*params)
        if rng.integers(0, 3) == 0:   # (again before the first result is read: the views are rewritten in place)
            params = PARAMS[1]
            out = win.compute(*params)
        ref = rec.reference(*params)
        wr.check_window(win, out, ref, f"seed {seed} {where}")
        for k, v in wr.facts(ref).items():
            info[k] += v
        info["window_checks"] += 1
        info["checks_after_chained_clear"] += int(chained)
        if clear:
            win.clear(keep_last=True)
            assert win.num_tables == 1
            rec.keep_last()
            chained = True
            info["chained_clears"] += 1

    def check(where):
        errs = compare(mgr, orc, where, depth_fixed=fixd) + episode_errors(mgr, orc, where)
        assert not errs, errs[:5]
        for out, want, at in pending:
            for k, img in out.items():
                got = img.cpu().numpy()
                assert got.shape == want[k].shape and np.array_equal(got, want[k]), \
                    (seed, where, "render", k, at, int((got != want[k]).sum()))
            info["renders"] += 1
            info["renders_after_later_step"] += int(t > at)
        pending.clear()

    def hush():
        """No shoot, no breed in the quiet worlds' current actions."""
        if not quiet:
            return
        cnt, off = orc.world_counts()
        rows = np.concatenate([orc.sensor_index()[off[w]:off[w] + cnt[w]] for w in sorted(quiet)])
        orc.column(pyoracle.COL_ACTION)[rows, 4:6] = 0
        mgr.action_tensor().to_torch()[torch.as_tensor(rows, dtype=torch.int64, device=mgr.device), 4:6] = 0

    win = open_window()
    for it in range(64):
        op = int(rng.integers(0, 22))
        if op < 7:
            if win.num_tables == HORIZON:
                window_check(f"op {it} full", clear=True)
            wh = bool(rng.integers(0, 2))
            mgr.write_synthetic_actions(1234, t, wh)
            orc.write_synthetic_actions(1234, t, wh)
            hush()
            wr.stamp(mgr, orc)
            rec.before_step()
            orc.step()
            assert orc.num_agents() <= win.max_rows, "the oracle's rows outgrew the window: size it larger"
            v = upload(rec.values(t + 1), win.max_rows)
            mgr.step()
            win.push(v)
            t += 1
            rec.table(t, stepped=True)
            quiet.clear()
            info["peak_population"] = max(info["peak_population"], int(orc.world_counts()[0].max()))
            info["peak_rows"] = max(info["peak_rows"], orc.num_agents())
        elif op in (7, 8):
            mgr.shift_observations()
            orc.shift_observations()
        elif op == 9:
            wh = bool(rng.integers(0, 2))
            mgr.write_synthetic_actions(4321, t, wh)
            orc.write_synthetic_actions(4321, t, wh)
            hush()
        elif op == 10:
            name, cid = COLUMNS[int(rng.integers(len(COLUMNS)))]
            prev = bool(rng.integers(0, 2))
            g, o = gpu_column(mgr, name, prev), orc.column(cid, prev)
            assert g.shape == o.shape and np.array_equal(bits(g), bits(o)), (it, name, prev)
        elif op == 11:
            prev = bool(rng.integers(0, 2))
            g = mgr.construct_obs(prev).cpu().numpy()
            o = _obs_rows_oracle(orc, prev, fixd)
            assert g.shape == o.shape and np.array_equal(bits(g), bits(o)), (it, "construct_obs", prev)
        elif op == 12:
            kind = int(rng.integers(0, 4))   # (half the draws: a checkpoint is a rare call)
            if kind < 2:
                window_check(f"op {it} before the load", clear=False)
                blob = mgr.save_checkpoint()
                if kind == 0:   # a fresh manager of a random class, and a new window
                    mgr = mb.SimManager(0, W, 69, 32, fix_depth_alias=fixd, exec_mode=exec_mode,
                                        agent_capacity=int(caps.choice(classes)))
                    mgr.load_checkpoint(blob)
                    assert mgr.schedule_info()["episodes_armed"]
                    win = open_window()
                else:           # the manager's own blob in place: the window is emptied
                    mgr.load_checkpoint(blob)
                    restart(win)
                flags = mgr.reset_tensor().to_torch()
        elif op in (13, 14):
            k = int(rng.integers(1, 6))
            worlds = rng.choice(W, size=k, replace=False).tolist()
            if rng.integers(0, 2):
                s = int(rng.choice(special))
                if s not in worlds:
                    worlds[0] = s
            eps = None if rng.integers(0, 2) else rng.integers(0, 8, size=k).tolist()
            mgr.reset_worlds(worlds, eps)
            orc.reset_worlds(worlds, eps)
        elif op == 15:
            w = int(rng.integers(W))
            v = 1 if rng.integers(0, 2) else int(rng.integers(0, 8)) + 2
            if rng.integers(0, 4) == 0:   # (sometimes a fresh view)
                flags = mgr.reset_tensor().to_torch()
            flags[w] = v
            oflags[w] = v
        elif op == 16:
            n = int(rng.choice([0, 3, 5]))
            mgr.set_episode_length(n)
            orc.set_episode_length(n)
        elif op == 17:
            if info["grown"] < 2 and mgr.agent_capacity < 1024:
                mgr.grow_capacity(2 * mgr.agent_capacity)
                info["grown"] += 1
                flags = mgr.reset_tensor().to_torch()   # (views do not follow a growth)
        elif op == 18:
            w = int(rng.integers(W))
            if rng.integers(0, 3) == 0:   # (a pending flag: the blob patched is an armed one)
                mgr.reset_worlds([w])
                orc.reset_worlds([w])
            st = orc.world_state(w)
            pos, rot = st["xy"].copy(), st["rot"].copy()
            pos[[0, 1]] = pos[[1, 0]]
            rot[[0, 1]] = rot[[1, 0]]
            # (only a scene the next step's clamp has already seen: see run_episode_sequence)
            if rng.integers(0, 2) and (pos[:, 0] <= 127).all() and (pos[:, 1] <= 95).all():
                window_check(f"op {it} before set_world_state", clear=False)
                mgr.set_world_state(w, pos, rot, st["food"])
                orc.set_world_state(w, pos, rot, st["food"])
                quiet.add(w)
                hush()
                restart(win)
        else:
            k = int(rng.integers(1, 4))
            worlds = rng.integers(0, W, size=k).tolist()   # (duplicates allowed)
            scale = int(rng.choice(SCALES, p=SCALE_P))
            keys = [key for key in RENDER_KEYS if rng.integers(0, 2)] or [RENDER_KEYS[int(rng.integers(3))]]
            out = mgr.render_worlds(worlds, scale, **{key: key in keys for key in RENDER_KEYS})
            want = wr.oracle_images(orc, worlds, scale, pal)
            pending.append((out, want, t))
        if it % 4 == 3:
            check(f"op {it}")
    window_check("end", clear=False)
    info["steps"] = t
    check("end")
    assert mgr.overflow() == 0 and orc.overflow() == 0
    # the sequence cannot pass vacuously (all from the reference side)
    assert info["window_checks"] >= 2 and info["checks_after_chained_clear"] >= 1, info
    assert info["alive"] >= 1 and info["deaths"] >= 1 and info["reset_cuts"] >= 1, info
    assert info["births"] >= 1 and info["renders_after_later_step"] >= 1, info
    return info


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_window_sequences_cpu_mode(seed):
    run_window_sequence(seed, exec_mode="cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_window_sequences(seed):
    """20 + seed worlds: the K1-finder mode."""
    run_window_sequence(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS_JOINED)
def test_window_sequences_joined_schedule(seed):
    """4100 worlds: the joined schedule with its value waits."""
    run_window_sequence(seed, W=4100)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS_SWAPPED)
def test_window_sequences_swapped_schedule(seed):
    """16400 worlds: K1 / K2 / the sensor, and so the producers the push and
    the render read, run on the internal stream."""
    run_window_sequence(seed, W=16400)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS_STREAM)
def test_window_sequences_on_a_side_stream(seed):
    """Every manager call (and every torch read and write of the test) under a
    non-default torch stream."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run_window_sequence(seed)
    s.synchronize()
