"""Device time of the per-seat advantage estimator (city_of_gold.turn_gae: cog_policy_gae, one
kernel) beside the same recursion written with torch ops, and its bytes per second as a fraction of
the engine's copy peak (cog_time_copy).

    python tools/policy_gae_time.py [--out profiles/policy_gae_time.txt] [--calls 200]

Per shape (T rows x n envs: 128 x 65,536, 128 x 8,192 and 20 x 65,536; seats in runs of 2 to 4 players,
a done in one row-env of 64, rewards NaN wherever not done, random values):
  kernel   _C.policy_gae_raw alone, `calls` calls queued behind a blocker (a chain of matmuls on the same
           stream) so the GPU runs them back to back; two events on the calling stream bracket them:
           device time per call, launch gaps included; the median of the repeated runs
  turn_gae city_of_gold.turn_gae(...), the checks and the two output allocations included, measured the
           same way
  torch    the recursion as a user would write it today: a Python loop over the T rows, each row a
           dozen ops on (n, 4) state tensors; checked equal to the kernel within the tests' tolerance
           (tests/gae_ref.py TOL) before anything is timed
Bytes per row-env: 22 read (the value, the agent byte, the done byte, 16 B of rewards) and 8 written
(advantage, return); the (n, 4) last values are read once.  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-eldorado_amd"))

TOL = 4 * 2.87e-6                     # tests/gae_ref.py TOL
SHAPES = ((128, 65536), (128, 8192), (20, 65536))
GAMMA, LAM = 0.99, 0.95


def torch_gae(torch, values, agents, rewards, dones, last_values, gamma, lam):
    """The torch-ops form of one turn_gae call."""
    T, n = values.shape
    dev = values.device
    nv = last_values.clone()
    A = torch.zeros((n, 4), device=dev)
    R = torch.zeros((n, 4), device=dev)
    adv = torch.empty((T, n), device=dev)
    ret = torch.empty((T, n), device=dev)
    seats = torch.arange(4, device=dev, dtype=torch.uint8)
    zero = torch.zeros((), device=dev)
    for t in range(T - 1, -1, -1):
        d = (dones[t] != 0)[:, None]
        nv = torch.where(d, zero, nv)
        A = torch.where(d, zero, A)
        R = torch.where(d, rewards[t], R)
        sel = (agents[t] & 3)[:, None] == seats
        v = values[t][:, None]
        cur = (R + gamma * nv - v) + (gamma * lam) * A
        adv[t] = torch.where(sel, cur, zero).sum(1)
        ret[t] = adv[t] + values[t]
        A = torch.where(sel, cur, A)
        nv = torch.where(sel, v, nv)
        R = torch.where(sel, zero, R)
    return adv, ret


def make_window(torch, gen, T, n, dev):
    """values, agents, rewards, dones, last_values on the device."""
    players = torch.randint(2, 5, (n,), generator=gen, device=dev)
    seat = torch.randint(0, 4, (n,), generator=gen, device=dev) % players
    dones = (torch.rand((T, n), generator=gen, device=dev) < 1.0 / 64).to(torch.uint8)
    turn = torch.rand((T, n), generator=gen, device=dev) < 0.3         # the seat's last row of its turn
    agents = torch.empty((T, n), dtype=torch.uint8, device=dev)
    for t in range(T):
        agents[t] = seat.to(torch.uint8)
        seat = torch.where(turn[t], (seat + 1) % players, seat)
        seat = torch.where(dones[t] != 0, torch.zeros_like(seat), seat)
    rewards = torch.randn((T, n, 4), generator=gen, device=dev)
    rewards = torch.where((dones != 0)[:, :, None], rewards, torch.full((), float("nan"), device=dev))
    values = torch.randn((T, n), generator=gen, device=dev)
    last_values = torch.randn((n, 4), generator=gen, device=dev)
    return values, agents, rewards, dones, last_values


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--torch-calls", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert args.calls >= 50 and args.runs >= 3
    import torch

    import city_of_gold as cg
    from city_of_gold import _city_of_gold as _C
    if not torch.cuda.is_available():
        raise SystemExit("policy_gae_time: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    peak = _C.time_copy(0, 1 << 30, 5)
    lines = [f"per-seat advantage estimator: device time per call, gamma {GAMMA} lam {LAM}; copy peak {peak:.0f} GB/s "
             "(cog_time_copy, 1 GiB, read + write)",
             f"{'T':>4} {'n':>6} | {'MB':>6} {'kernel us':>9} {'GB/s':>6} {'of peak':>7} {'turn_gae us':>11} | {'torch us':>9} "
             f"{'torch/kernel':>12} | {'max |kernel - torch|':>20}"]
    detail = []
    blocker = torch.randn(4096, 4096, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)

    def queued(fn, calls):
        """us per call of `calls` calls run back to back behind a blocker: the runs, sorted."""
        out = []
        for _ in range(args.runs):
            m = blocker
            for _ in range(12):
                m = torch.tanh(m @ m)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / calls)
        return sorted(out)

    for T, n in SHAPES:
        values, agents, rewards, dones, last_values = make_window(torch, gen, T, n, dev)
        adv = torch.empty((T, n), device=dev)
        ret = torch.empty((T, n), device=dev)
        stream = int(torch.cuda.current_stream(dev).cuda_stream)

        def kernel():
            _C.policy_gae_raw(T, n, values.data_ptr(), n, agents.data_ptr(), n, rewards.data_ptr(), 4 * n, dones.data_ptr(), n,
                              last_values.data_ptr(), GAMMA, LAM, adv.data_ptr(), ret.data_ptr(), 0, stream)

        def face():
            cg.turn_gae(values, agents, rewards, dones, last_values, gamma=GAMMA, lam=LAM)

        def composed():
            with torch.no_grad():
                return torch_gae(torch, values, agents, rewards, dones, last_values, GAMMA, LAM)

        kernel()
        t_adv, t_ret = composed()
        torch.cuda.synchronize()
        err = max((adv - t_adv).abs().max().item(), (ret - t_ret).abs().max().item())
        if not (torch.isfinite(adv).all().item() and err <= TOL):
            raise SystemExit(f"policy_gae_time: T={T} n={n}: the kernel and the torch loop differ by {err:.3g} (> {TOL:.3g})")
        for f in (kernel, face):
            for _ in range(5):
                f()
        composed()
        torch.cuda.synchronize()
        t_k, t_f = queued(kernel, args.calls), queued(face, args.calls)
        t_t = queued(composed, args.torch_calls)
        nbytes = 30 * T * n + 16 * n
        k = median(t_k)
        gbs = nbytes / k * 1e-3
        lines.append(f"{T:>4} {n:>6} | {nbytes / 1e6:>6.1f} {k:>9.2f} {gbs:>6.0f} {gbs / peak:>7.2f} {median(t_f):>11.2f} | "
                     f"{median(t_t):>9.0f} {median(t_t) / k:>12.0f} | {err:>20.3g}")
        for label, t in (("kernel", t_k), ("turn_gae", t_f), ("torch", t_t)):
            detail.append(f"  {T:>4} {n:>6} {label:>9} runs (us per call): {' '.join(f'{q:.2f}' for q in t)}")
    text = "\n".join(lines + ["medians of the runs below; torch/kernel: the torch loop's time over the kernel's"] + detail) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
