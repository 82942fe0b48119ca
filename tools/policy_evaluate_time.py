"""Device time of the policy evaluator (city_of_gold.policy_evaluate: cog_policy_evaluate and its
backward) beside the same maths written with torch ops and differentiated by torch's autograd, and
its bytes per second as a fraction of the engine's copy peak (cog_time_copy).

    python tools/policy_evaluate_time.py [--out profiles/policy_evaluate_time.txt] [--calls 400]

Per shape (65,536 and 8,192 rows, float32 and bfloat16 logits, ld = 92, dense random masks -- about
half of every head valid -- and actions sampled from them by sample_policy):
  fwd      the forward kernel alone (_C.policy_evaluate_raw), `calls` calls queued behind a blocker (a
           chain of matmuls on the same stream) so the GPU runs them back to back; two events on the
           calling stream bracket them: device time per call, launch gaps included; the median of the
           repeated runs
  fwd+bwd  the forward and the backward kernel alternating, measured the same way, per pair
  autograd policy_evaluate(...) and torch.autograd.backward through the torch.autograd.Function: what
           a trainer pays per update, torch's own bookkeeping included (per pair, median)
  torch    masked log_softmax, gather and entropy per head with torch ops, forward (under no_grad) and
           forward + backward, as a user would write it today (median)
Bytes per row, forward: the logits (368 / 184), the 128-B ActionMask record, 5 action bytes, logp and
entropy; forward + backward: the logits and the mask record twice, the actions twice, logp and
entropy written and their gradients read, the gradient row written (368 / 184).  Needs a GPU; there is
no CPU fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-eldorado_amd"))

HEADS = ((0, 22), (22, 22), (44, 22), (66, 7), (73, 19))


def torch_compose(torch, logits, actions, masks):
    """The torch-ops form of one policy_evaluate call."""
    n = logits.shape[0]
    valid = masks[:, :92] != 0
    l = logits.float().masked_fill(~valid, float("-inf"))
    logp = torch.zeros(n, device=logits.device)
    ent = torch.zeros(n, device=logits.device)
    for h, (off, k) in enumerate(HEADS):
        v = valid[:, off:off + k]
        some = v.any(1)
        lh = torch.where(some[:, None], l[:, off:off + k], torch.zeros((), device=logits.device))
        lsm = torch.log_softmax(lh, 1)
        p = lsm.exp()
        a = actions[:, h].long()
        logp = logp + torch.where(some, lsm.gather(1, a[:, None]).squeeze(1), torch.zeros_like(logp))
        ent = ent - torch.where(some, torch.where(v, p * lsm.masked_fill(~v, 0.0), torch.zeros_like(p)).sum(1),
                                torch.zeros_like(ent))
    return logp, ent


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--torch-calls", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert args.calls >= 100 and args.runs >= 3
    import torch

    import city_of_gold as cg
    from city_of_gold import _city_of_gold as _C
    if not torch.cuda.is_available():
        raise SystemExit("policy_evaluate_time: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    peak = _C.time_copy(0, 1 << 30, 5)
    lines = [f"policy evaluator: device time per call; copy peak {peak:.0f} GB/s (cog_time_copy, 1 GiB, read + write)",
             f"{'rows':>6} {'dtype':>5} | {'B/row':>5} {'fwd us':>7} {'GB/s':>6} {'of peak':>7} {'torch us':>9} {'torch/fwd':>9} | "
             f"{'B/row':>5} {'f+b us':>7} {'GB/s':>6} {'of peak':>7} {'autograd us':>11} {'torch us':>9} {'torch/f+b':>9}"]
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

    for n in (65536, 8192):
        masks = (torch.rand((n, 128), generator=gen, device=dev) < 0.5).to(torch.uint8)
        smp = cg.vec.get_vec_sampler(n)(7, device=0)
        logp = torch.empty(n, device=dev)
        ent = torch.empty(n, device=dev)
        g_lp = torch.randn(n, generator=gen, device=dev)
        g_en = torch.randn(n, generator=gen, device=dev)
        for dt, code in ((torch.float32, 0), (torch.bfloat16, 1)):
            logits = (torch.randn((n, 92), generator=gen, device=dev) * 3).clamp(-8, 8).to(dt)
            actions = smp.sample_policy(logits, None, masks)[0][:, :5].contiguous()
            grad = torch.empty((n, 92), dtype=dt, device=dev)
            stream = int(torch.cuda.current_stream(dev).cuda_stream)
            common = (n, logits.data_ptr(), code, 92, actions.data_ptr(), 5, masks.data_ptr())

            def fwd():
                _C.policy_evaluate_raw(*common, logp.data_ptr(), ent.data_ptr(), 0, 0, 0, 0, stream, False)

            def bwd():
                _C.policy_evaluate_raw(*common, 0, 0, g_lp.data_ptr(), g_en.data_ptr(), grad.data_ptr(), 0, stream, True)

            def both():
                fwd()
                bwd()
            leaf = logits.clone().requires_grad_(True)

            def autograd():
                leaf.grad = None
                lp, en = cg.policy_evaluate(leaf, actions, masks)
                torch.autograd.backward([lp, en], [g_lp, g_en])

            def torch_fwd():
                with torch.no_grad():
                    torch_compose(torch, logits, actions, masks)

            def torch_both():
                leaf.grad = None
                lp, en = torch_compose(torch, leaf, actions, masks)
                torch.autograd.backward([lp, en], [g_lp, g_en])
            for f in (fwd, both, autograd, torch_fwd, torch_both):
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            t_fwd, t_both = queued(fwd, args.calls), queued(both, args.calls // 2)
            t_auto = queued(autograd, args.calls // 4)
            t_tf, t_tb = queued(torch_fwd, args.torch_calls), queued(torch_both, args.torch_calls)
            es = logits.element_size()
            b_fwd = 92 * es + 128 + 5 + 8
            b_both = 2 * (92 * es + 128 + 5) + 16 + 92 * es
            f, b = median(t_fwd), median(t_both)
            gf, gb = n * b_fwd / f * 1e-3, n * b_both / b * 1e-3
            name = "f32" if code == 0 else "bf16"
            lines.append(f"{n:>6} {name:>5} | {b_fwd:>5} {f:>7.2f} {gf:>6.0f} {gf / peak:>7.2f} {median(t_tf):>9.1f} "
                         f"{median(t_tf) / f:>9.0f} | {b_both:>5} {b:>7.2f} {gb:>6.0f} {gb / peak:>7.2f} {median(t_auto):>11.1f} "
                         f"{median(t_tb):>9.1f} {median(t_tb) / b:>9.0f}")
            for label, t in (("fwd", t_fwd), ("fwd+bwd", t_both), ("autograd", t_auto), ("torch fwd", t_tf), ("torch fwd+bwd", t_tb)):
                detail.append(f"  {n:>6} {name:>5} {label:>13} runs (us per call): {' '.join(f'{q:.2f}' for q in t)}")
    text = "\n".join(lines + ["medians of the runs below; torch/fwd and torch/f+b: the torch composition's time over the kernels'"]
                     + detail) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
