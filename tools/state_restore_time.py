"""Time of envs.snapshot() and envs.restore() (cog_env_snapshot / cog_env_restore: k_state_save,
k_state_restore) beside what they replace or compete with: observations.clone(), and a full reset
of the batch, which is how one gets a known state without them.

    python tools/state_restore_time.py [--out profiles/state_restore_time.txt] [--calls 30]

65,536 envs (4 players, 3 pieces, HARD, 40 full-dynamics steps after the reset), one handle without
host views (a restore then publishes nothing; the last restore row is the same handle once it has
them -- device_tensors() allocates them -- where a restore also publishes every record and copies
every map to the host, 1.1 GB over PCIe):
  snapshot        the save alone, `calls` calls queued back to back on the envs' stream (it does not
                  wait on the host); two events ordered around them through wait_stream /
                  signal_stream: device time per call, launch gaps included
  restore         src=None, identity src (int32 arange) and a one-source fork (src all 7).  A restore
                  returns complete (it ends like invalidate_device), so calls cannot be queued: each
                  call is bracketed by two events of its own (`span`: from the envs' stream taking
                  the call's first kernel to its last, which for a src includes the index check and
                  the host's wait for it); `wall` is the host clock around a call of its own
  clone           t["observations"].clone() on torch's stream, queued back to back: 17,216 B read and
                  written per env
  reset           envs.reset(...) of the whole batch, host clock (it is synchronous)
Medians of the repeated runs; every run is listed.  Bytes per env: a snapshot reads and writes
4,032 B; a restore reads 4,032 B and writes 1,680 B of records, the 2,304-B code grid and the
16,128-B map observation (plus the old map's box in the generation grid, about 2.5 KB).
Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-eldorado_amd"))

N, PLAYERS = 65536, 4
SNAP_BYTES, RESTORE_WRITES = 4032, 1680 + 2304 + 16128


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--resets", type=int, default=5)
    ap.add_argument("--envs", type=int, default=N)
    args = ap.parse_args()
    assert args.calls >= 20 and args.runs >= 3 and args.resets >= 3
    import torch

    import city_of_gold as cg
    from city_of_gold import _city_of_gold as _C
    if not torch.cuda.is_available():
        raise SystemExit("state_restore_time: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    n = args.envs
    peak = _C.time_copy(0, 1 << 30, 5)
    env, smp = cg.vec.get_vec_env(n)(device=0), cg.vec.get_vec_sampler(n)(7, device=0)

    def reset():
        env.reset(7, PLAYERS, 3, cg.HARD, 100000, False)

    reset()
    t_reset = []
    for _ in range(args.resets):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reset()
        t_reset.append((time.perf_counter() - t0) * 1e6)
    runner = cg.vec.get_runner(n)(env, smp, None, device_views=True, stored_masks=True)
    runner.rollout(40)
    runner.sync()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    snap = env.snapshot()
    torch.cuda.synchronize()

    def bracket(fn, calls):
        """Device us per call of `calls` calls of fn on the envs' stream, between two torch events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        env.wait_stream(stream)
        for _ in range(calls):
            fn()
        env.signal_stream(stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    def save():
        _C.VecEnvBase.snapshot_raw(env, snap, -1)

    def each_call(fn, calls):
        fn()
        spans, walls = [], []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            walls.append((time.perf_counter() - t0) * 1e6)
            spans.append(bracket(fn, 1))
        return sorted(spans), sorted(walls)

    ident = torch.arange(n, dtype=torch.int32, device=dev)
    one = torch.full((n,), 7, dtype=torch.int32, device=dev)
    restores = (("restore src=None", lambda: env.restore(snap, stream=-1)),
                ("restore identity src", lambda: env.restore(snap, ident, stream=-1)),
                ("one-source fork", lambda: env.restore(snap, one, stream=-1)))
    # the handle has no host views yet (device_tensors below gives it some: cog_env_shard_views)
    for f in (save,) + tuple(r[1] for r in restores[:2]):
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t_save = sorted(bracket(save, args.calls) for _ in range(args.runs))
    rows = [(label,) + each_call(fn, args.calls) for label, fn in restores]
    # the same calls change nothing: a restore of the snapshot, then one through the identity
    env.restore(snap)
    t = cg.device_tensors(env)
    torch.cuda.synchronize()
    before = {nm: t[nm].clone() for nm in cg.DEVICE_VIEWS}
    env.snapshot(out=snap)
    env.restore(snap, ident)
    torch.cuda.synchronize()
    for nm in cg.DEVICE_VIEWS:
        if not torch.equal(t[nm], before[nm]):
            raise SystemExit(f"state_restore_time: {nm} changed under snapshot + restore")
    rows.append(("  with host views",) + each_call(restores[0][1], 5))
    obs = t["observations"]

    def clone():
        return obs.clone()

    for _ in range(5):
        clone()
    torch.cuda.synchronize()
    e = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            clone()
        e1.record()
        torch.cuda.synchronize()
        e.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    t_clone = sorted(e)
    c, s, rs = median(t_clone), median(t_save), median(t_reset)
    clone_bytes, save_bytes, restore_bytes = 2 * 17216 * n, 2 * SNAP_BYTES * n, (SNAP_BYTES + RESTORE_WRITES) * n
    lines = [f"state snapshots: time per call, {n} envs, {PLAYERS} players, HARD, 40 steps after the reset, a handle without host views; "
             f"copy peak {peak:.0f} GB/s (cog_time_copy, 1 GiB, read + write)",
             f"{'':>22} | {'us':>9} {'MB':>7} {'GB/s':>6} {'of peak':>7} | {'clone/this':>10} | {'wall us':>8}",
             f"{'observations.clone()':>22} | {c:>9.1f} {clone_bytes / 1e6:>7.0f} {clone_bytes / c * 1e-3:>6.0f} "
             f"{clone_bytes / c * 1e-3 / peak:>7.2f} | {1.0:>10.2f} |",
             f"{'snapshot':>22} | {s:>9.1f} {save_bytes / 1e6:>7.0f} {save_bytes / s * 1e-3:>6.0f} "
             f"{save_bytes / s * 1e-3 / peak:>7.2f} | {c / s:>10.2f} |"]
    for label, spans, walls in rows:
        k = median(spans)
        nbytes = restore_bytes if label != "one-source fork" else RESTORE_WRITES * n
        lines.append(f"{label:>22} | {k:>9.1f} {nbytes / 1e6:>7.0f} {nbytes / k * 1e-3:>6.0f} {nbytes / k * 1e-3 / peak:>7.2f} | "
                     f"{c / k:>10.2f} | {median(walls):>8.1f}")
    lines.append(f"{'reset of the batch':>22} | {rs:>9.0f} {'':>7} {'':>6} {'':>7} | {c / rs:>10.4f} | {rs:>8.0f}   "
                 f"({n / rs:.1f} M resets/s)")
    lines.append("medians of the runs below; MB: bytes read + written from HBM (the fork's reads come from L2: its writes alone); "
                 "clone/this: the clone's time over this one's (above 1: faster than the clone)")
    detail = [f"  {'clone':>22} runs (us per call): {' '.join(f'{q:.1f}' for q in t_clone)}",
              f"  {'snapshot':>22} runs (us per call): {' '.join(f'{q:.1f}' for q in t_save)}"]
    for label, spans, walls in rows:
        detail.append(f"  {label:>22} span, every call (us): {' '.join(f'{q:.0f}' for q in spans)}")
        detail.append(f"  {label:>22} wall, every call (us): {' '.join(f'{q:.0f}' for q in walls)}")
    detail.append(f"  {'reset':>22} every call (us): {' '.join(f'{q:.0f}' for q in sorted(t_reset))}")
    text = "\n".join(lines + detail) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
