"""Device time of the policy sampler (samplers.sample_policy / cog_sampler_sample_policy) beside the
same sampling written with torch ops, and its bytes per second as a fraction of the engine's copy
peak (cog_time_copy).

    python tools/policy_sample_time.py [--out profiles/policy_sample_time.txt] [--calls 400]

Per shape (65,536 and 8,192 envs, float32 and bfloat16 logits, ld = 92, dense random masks from a
device pointer -- about half of every head valid, the most work per env the kernel can get):
  queued   `calls` calls queued behind a blocker (a chain of matmuls on the same stream) so the GPU
           runs them back to back; two events on the calling stream bracket them: device time per
           call, launch gaps between consecutive calls included
  paired   an event pair around every call, GPU otherwise idle: the median over the calls
  torch    masked softmax, multinomial, gather, pack, per head, as a user would write it today
Bytes per env: the logits (368 / 184), the 128-B ActionMask record, the 4-B sampler state read and
written, 8 B of ActionData, logp and entropy.  Needs a GPU; there is no CPU fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-eldorado_amd"))

HEADS = ((0, 22), (22, 22), (44, 22), (66, 7), (73, 19))


def torch_compose(torch, logits, masks, acts):
    """The torch-ops form of one sample_policy call (no minstd: torch's own generator)."""
    n = logits.shape[0]
    valid = masks[:, :92] != 0
    l = logits.float().masked_fill(~valid, float("-inf"))
    logp = torch.zeros(n, device=logits.device)
    ent = torch.zeros(n, device=logits.device)
    for h, (off, k) in enumerate(HEADS):
        some = valid[:, off:off + k].any(1)
        lh = torch.where(some[:, None], l[:, off:off + k], torch.zeros((), device=logits.device))
        lsm = torch.log_softmax(lh, 1)
        p = lsm.exp()
        a = torch.multinomial(p, 1).squeeze(1)
        a = torch.where(some, a, torch.zeros_like(a))
        logp += torch.where(some, lsm.gather(1, a[:, None]).squeeze(1), torch.zeros_like(logp))
        ent -= torch.where(some, torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(1), torch.zeros_like(ent))
        acts[:, h] = a.to(torch.uint8)
    return acts, logp, ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--torch-calls", type=int, default=50)
    args = ap.parse_args()
    assert args.calls >= 200
    import torch

    import city_of_gold as cg
    from city_of_gold import _city_of_gold as _C
    if not torch.cuda.is_available():
        raise SystemExit("policy_sample_time: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    peak = _C.time_copy(0, 1 << 30, 5)
    lines = [f"policy sampler: device time per call; copy peak {peak:.0f} GB/s (cog_time_copy, 1 GiB, read + write)",
             f"{'envs':>6} {'dtype':>5} {'B/env':>5} {'queued us':>9} {'GB/s':>6} {'of peak':>7} {'paired us':>9} {'torch us':>9} {'torch/kernel':>12}"]
    blocker = torch.randn(4096, 4096, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (65536, 8192):
        masks = (torch.rand((n, 128), generator=gen, device=dev) < 0.5).to(torch.uint8)
        smp = cg.vec.get_vec_sampler(n)(7, device=0)
        logp = torch.empty(n, device=dev)
        ent = torch.empty(n, device=dev)
        for dt, code in ((torch.float32, 0), (torch.bfloat16, 1)):
            logits = (torch.randn((n, 92), generator=gen, device=dev) * 3).clamp(-8, 8).to(dt)
            stream = int(torch.cuda.current_stream(dev).cuda_stream)

            def call():
                smp.sample_policy_raw(logits.data_ptr(), code, 92, 2, None, masks.data_ptr(), logp.data_ptr(),
                                      ent.data_ptr(), 0, stream)
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            queued = []
            for _ in range(3):                             # back to back behind a blocker
                m = blocker
                for _ in range(12):
                    m = torch.tanh(m @ m)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                queued.append(e0.elapsed_time(e1) * 1e3 / args.calls)
            pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
            for a, b in pairs:                             # one pair per call, GPU otherwise idle
                a.record()
                call()
                b.record()
            torch.cuda.synchronize()
            paired = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)[len(pairs) // 2]
            acts = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            for _ in range(5):
                torch_compose(torch, logits, masks, acts)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.torch_calls):
                torch_compose(torch, logits, masks, acts)
            e1.record()
            torch.cuda.synchronize()
            t_torch = e0.elapsed_time(e1) * 1e3 / args.torch_calls
            per_env = 92 * logits.element_size() + 128 + 8 + 8 + 8
            us = min(queued)
            gbs = n * per_env / us * 1e-3
            lines.append(f"{n:>6} {'f32' if code == 0 else 'bf16':>5} {per_env:>5} {us:>9.2f} {gbs:>6.0f} {gbs / peak:>7.2f} "
                         f"{paired:>9.2f} {t_torch:>9.1f} {t_torch / us:>12.0f}")
            lines.append(f"       queued runs (us per call): {' '.join(f'{q:.2f}' for q in queued)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
