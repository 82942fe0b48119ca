"""city_of_gold -- MI355X-native drop-in for the reference `city_of_gold` pybind11 module.

Same surface as the reference (src/pybind/common.cpp:5-37, src/pybind/vectorized.cpp:8-21,
include/pybind/vectorized.h:163-275):

    import city_of_gold as cg
    envs = cg.vec.get_vec_env(N)()           # class vec_cog_env_N
    samplers = cg.vec.get_vec_sampler(N)(seed)
    runner = cg.vec.get_runner(N)(envs, samplers, n_threads)
    envs.reset(seed, 4, 3, cg.Difficulty.EASY, 100000, False)

Differences, all additive: any N is accepted (the reference stops at 256 and only offers
N in {0..8, 16, 32, ..., 256}); input arrays are length/record-size checked (ValueError instead
of an out-of-bounds read); views keep their owner alive.  Runners accept two extra keyword
arguments: device_views=True keeps outputs in HBM (no per-sync host copy) and
stored_masks=True samples from the current agent's stored mask (full game dynamics); samplers
accept first_index= for a rank's block of a larger batch (city_of_gold.shard), and have
sample_policy(logits, envs, masks): masked categorical actions, their joint log-probability and
entropy from a policy's logits on the GPU, feeding envs.step_device with no host round trip.
For the update, policy_evaluate(logits, actions, masks) gives the log-probability of recorded
actions and the entropy under new logits, with gradients (a torch.autograd.Function over two HIP
kernels), and mask_records(envs, source) copies the masks a trainer has to record with them.
turn_gae(values, agents, rewards, dones, last_values) turns a recorded window into per-seat
advantages and returns (GAE over each seat's own rows of each episode), one HIP kernel.
policy_features(envs, radius) gives the network's input: a flat (n, 208) tensor and an
(n, 10, W, W) window of the map centred on the seat's own cell, seen from the acting seat (or any
seat), positions included, float32 or bfloat16, one HIP kernel between the step and the network.
envs.snapshot() saves the complete state of every env on the GPU (an EnvSnapshot) and
envs.restore(snap, src) puts it back, or forks it: env j takes snapshot env src[j], for playouts,
tree search and replay.

All computation runs in libcog_hip.so on a gfx950 GPU.  There is no CPU fallback: creating an
environment without a usable device raises RuntimeError.
"""
from __future__ import annotations

import os
import sys
import types

# torch (ROCm) and this engine load the same HIP runtime (SONAME libamdhip64.so.7).  torch rejects
# a runtime another library has already brought up ("No HIP GPUs are available"), while the
# engine is happy with torch's, so when torch is installed its GPU side is brought up first.
# COG_NO_TORCH=1 skips this (torch interop, e.g. device_tensors, then needs torch initialised
# before the first environment is created).
if not os.environ.get("COG_NO_TORCH"):
    try:
        import torch as _torch
        if _torch.cuda.is_available():
            _torch.cuda.init()
    except Exception:
        pass

from . import _city_of_gold as _C

Difficulty = _C.Difficulty
EASY, MEDIUM, HARD = _C.EASY, _C.MEDIUM, _C.HARD
# record classes (single_env.cpp:34-85); each also acts as its numpy dtype (np.zeros(n, dtype=cg.ActionData))
from .records import (ActionData, ActionMask, DeckObs, Info, ObsData, PlayerData, PlayerObservation,  # noqa: E402
                      SharedObservation, action_sampler)
device_count = _C.device_count
EnvSnapshot = _C.EnvSnapshot           # envs.snapshot() / envs.restore(snap, src): state save, restore and fork

VEC_ENV_CLS = "vec_cog_env_"
VEC_SAMPLER_CLS = "vec_sampler_"
VEC_RUNNER_CLS = "vec_runner_"

vec = types.ModuleType("city_of_gold.vec", "Vectorized utilities")
# Q28: the reference binds samplers into `vec.env` and envs into `vec.sampler`
# (include/pybind/vectorized.h:260-273, call order vs. parameter names); the getters are right.
vec.env = types.ModuleType("city_of_gold.vec.env", "Vectorized environments")
vec.sampler = types.ModuleType("city_of_gold.vec.sampler", "Vectorized action samplers")
vec.runner = types.ModuleType("city_of_gold.vec.runner", "Vectorized runners")
for _m in (vec, vec.env, vec.sampler, vec.runner):
    sys.modules[_m.__name__] = _m


def _check_n(n):
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise TypeError("number of environments must be a non-negative int")
    return int(n)


def _make_env_cls(n):
    def __init__(self, device=None):
        _C.VecEnvBase.__init__(self, n, device)

    def step_device(self, d_actions, stream=None):
        """step() with ActionData records in device memory (a torch tensor's data_ptr()),
        ordered after torch's current stream, or after `stream` (a hipStream_t handle, 0 = the
        null stream; -1: no ordering)."""
        if stream is None:
            # torch's current stream ON THE ENV'S DEVICE (a stream of another GPU cannot order it)
            stream = stream_handle(_C.VecEnvBase.shard_info(self, 0)[2])
        _C.VecEnvBase.step_device(self, d_actions, -1 if stream is None else int(stream))

    def invalidate_device(self, stream=None):
        """After writing device records (device_tensors / DLPack views): the next step takes them
        as written, as the reference's views alias its live state.  Ordered after torch's current
        stream on the env's device (or after `stream`, a hipStream_t handle; -1: no ordering)."""
        if stream is None and self.num_shards == 1:
            stream = stream_handle(_C.VecEnvBase.shard_info(self, 0)[2])
        _C.VecEnvBase.invalidate_device(self, -1 if stream is None else int(stream))

    def snapshot(self, out=None, stream=None):
        """The complete state of every env, saved into device memory: an EnvSnapshot (about 4 KB per
        env, one piece per shard on the shard's device).  out: an EnvSnapshot of the same layout to
        write into (nothing is allocated); None for a new one.  The copy is enqueued behind the envs'
        queued work (and, for a single-shard env, behind torch's current stream, or `stream`; -1: no
        ordering); nothing waits on the host, so it can sit between two runner.rollout launches.

        Saved: everything a step reads -- records, masks, counters, the map, each env's generator, seed,
        n_players, max_steps and turn counter.  Not saved: the auto-reset switch, samplers, timing."""
        if out is None:
            out = EnvSnapshot(self)
        elif not isinstance(out, EnvSnapshot):
            raise ValueError("snapshot: out must be an EnvSnapshot")
        if stream is None and self.num_shards == 1:
            stream = stream_handle(_C.VecEnvBase.shard_info(self, 0)[2])
        _C.VecEnvBase.snapshot_raw(self, out, -1 if stream is None else int(stream))
        return out

    def restore(self, snap, src=None, stream=None):
        """The envs take the state held in `snap` and go on from it as the saved envs would have, under
        every driver (step, step_device, runners, rollouts, auto-resets).

        src=None: env i takes snapshot env i; the snapshot's shard layout (counts and devices) must
        equal the envs'.  src: an (n,) int32, uint32 or int64 torch tensor on the envs' device, env j
        takes snapshot env src[j]; indices may repeat (a fork), the snapshot may hold more or fewer envs
        than the handle; envs and snapshot must be single-shard on one device.  The indices are checked
        on the device before anything is written, and the call waits for that check.  A refused call
        (ValueError) leaves the envs untouched.

        Ordered after the envs' queued work and torch's current stream (or `stream`; -1: no ordering);
        like invalidate_device() it returns with the host views (when there are any) refreshed."""
        if not isinstance(snap, EnvSnapshot):
            raise ValueError("restore: snap must be an EnvSnapshot")
        d_src, kind, n_src = 0, 0, 0
        if src is not None:
            import torch
            if self.num_shards != 1 or len(snap.devices) != 1:
                raise ValueError("restore: src needs a single-shard env and a single-shard snapshot")
            dev = _C.VecEnvBase.shard_info(self, 0)[2]
            kinds = {torch.int32: 0, torch.int64: 2}
            if hasattr(torch, "uint32"):
                kinds[torch.uint32] = 1
            if not isinstance(src, torch.Tensor):
                raise ValueError("restore: src must be a torch tensor")
            if src.dtype not in kinds:
                raise ValueError(f"restore: src dtype {src.dtype} is not int32, uint32 or int64")
            if src.device.type != "cuda" or src.device.index != dev:
                raise ValueError(f"restore: src is on device {src.device}, the envs are on GPU {dev}")
            if tuple(src.shape) != (n,) or not src.is_contiguous():
                raise ValueError(f"restore: src has shape {tuple(src.shape)}, expected a contiguous ({n},)")
            d_src, kind, n_src = src.data_ptr(), kinds[src.dtype], n
            if n == 0:
                d_src = 0
                if snap.n != 0:
                    return
        if stream is None and self.num_shards == 1:
            stream = stream_handle(_C.VecEnvBase.shard_info(self, 0)[2])
        _C.VecEnvBase.restore_raw(self, snap, d_src, kind, n_src, -1 if stream is None else int(stream))

    doc = (f"Vectorized city of gold environment for {n} environments.\n\n"
           "reset() must be called first to initialize the environments before stepping.")
    return type(VEC_ENV_CLS + str(n), (_C.VecEnvBase,), {"__init__": __init__, "__doc__": doc,
                                                         "step_device": step_device,
                                                         "invalidate_device": invalidate_device,
                                                         "snapshot": snapshot, "restore": restore,
                                                         "__module__": "city_of_gold.vec.sampler"})


def _make_sampler_cls(n):
    def __init__(self, seed=None, device=None, *, first_index=0):
        """first_index (an addition): the batch is envs [first_index, first_index + n) of a larger
        one (a rank's shard, city_of_gold.shard), so sampler i is seeded seed + first_index + i
        unwrapped, as in the whole batch (vec_sampler.h:9-13)."""
        _C.VecSamplerBase.__init__(self, n, seed, device, first_index)

    def sample_policy(self, logits, envs=None, masks="selected", *, greedy=False, stream=None):
        """Masked categorical actions from a policy's logits, one fused kernel on the GPU (an
        addition: the reference samples uniformly only).

        logits: torch tensor on the sampler's device, shape (n, 92) in ActionMask byte order (play
        0..21, play_special 22..43, remove 44..65, move 66..72, get_from_shop 73..91), float32 or
        bfloat16, stride(1) == 1, stride(0) >= 92.  masks: "selected" (envs' selected masks),
        "stored" (the current agent's stored mask: full dynamics) or an (n, 128) uint8 device
        tensor of ActionMask records.  greedy=True takes the valid entry with the largest logit and
        leaves the sampler's state alone.  The kernel is ordered after `stream` (default: torch's
        current stream on that device) and, with envs' masks, after the envs' queued work; what is
        queued on that stream afterwards (reading the results, envs.step_device(actions)) runs
        after it.  Nothing waits on the host.

        Returns (actions, logp, entropy): the sampler's device actions, (n, 64) uint8, the memory
        device_tensors(...)["actions"] aliases, and two new float32 (n,) tensors: the joint
        log-probability of the five heads and their summed entropy (NaN for an env with a +inf
        logit, or nothing but -inf / NaN, on a head's valid entries; its action is still legal)."""
        import torch
        if self.num_shards != 1:
            raise ValueError(f"sample_policy of a {self.num_shards}-shard sampler: it needs a single-shard "
                             "sampler (one device)")
        if not isinstance(logits, torch.Tensor):
            raise ValueError("sample_policy: logits must be a torch tensor")
        dev = self.device
        if logits.device.type != "cuda" or logits.device.index != dev:
            raise ValueError(f"sample_policy: logits are on device {logits.device}, the sampler is on GPU {dev}")
        if logits.dim() != 2 or tuple(logits.shape) != (n, 92):
            raise ValueError(f"sample_policy: logits have shape {tuple(logits.shape)}, expected ({n}, 92)")
        dtypes = {torch.float32: 0, torch.bfloat16: 1}
        if logits.dtype not in dtypes:
            raise ValueError(f"sample_policy: logits dtype {logits.dtype} is neither float32 nor bfloat16")
        if n and (logits.stride(1) != 1 or (n > 1 and logits.stride(0) < 92)):
            raise ValueError(f"sample_policy: logits strides {tuple(logits.stride())}: the inner stride must be 1 "
                             "and the row stride at least 92")
        ld = logits.stride(0) if n > 1 else 92
        d_masks = 0
        if isinstance(masks, str):
            if masks not in ("selected", "stored"):
                raise ValueError(f"sample_policy: masks {masks!r} is not 'selected', 'stored' or a tensor")
            if envs is None:
                raise ValueError(f"sample_policy: masks={masks!r} needs the envs whose masks they are (envs=None)")
            source = 0 if masks == "selected" else 1
        else:
            if (not isinstance(masks, torch.Tensor) or masks.device != logits.device or masks.dtype != torch.uint8
                    or tuple(masks.shape) != (n, 128) or not masks.is_contiguous()):
                raise ValueError(f"sample_policy: mask records must be a contiguous ({n}, 128) uint8 tensor on "
                                 "the logits' device")
            source, envs, d_masks = 2, None, masks.data_ptr()
        if stream is None:
            stream = stream_handle(dev)
        actions = torch.from_dlpack(self.dlpack())
        logp = torch.empty(n, dtype=torch.float32, device=logits.device)
        entropy = torch.empty(n, dtype=torch.float32, device=logits.device)
        _C.VecSamplerBase.sample_policy_raw(self, logits.data_ptr(), dtypes[logits.dtype], ld, source, envs, d_masks,
                                            logp.data_ptr(), entropy.data_ptr(), 1 if greedy else 0,
                                            -1 if stream is None else int(stream))
        return actions, logp, entropy

    return type(VEC_SAMPLER_CLS + str(n), (_C.VecSamplerBase,), {"__init__": __init__,
                                                                 "sample_policy": sample_policy,
                                                                 "__module__": "city_of_gold.vec.env"})


def _make_runner_cls(n):
    def __init__(self, env, sampler, n_threads=None, device_views=False, stored_masks=False):
        if env.num_envs != n:
            raise ValueError(f"runner for {n} envs got an env batch of {env.num_envs}")
        _C.RunnerBase.__init__(self, env, sampler, n_threads, device_views, stored_masks)

    return type(VEC_RUNNER_CLS + str(n), (_C.RunnerBase,), {"__init__": __init__,
                                                            "__module__": "city_of_gold.vec.runner"})


def _getter(module, prefix, factory):
    def get(n):
        n = _check_n(n)
        name = prefix + str(n)
        cls = getattr(module, name, None)
        if cls is None:
            cls = factory(n)
            setattr(module, name, cls)
        return cls

    return get


DEVICE_VIEWS = ("observations", "selected_action_masks", "rewards", "dones", "agent_selection", "infos")


def device_tensors(env, sampler=None, shard=None):
    """Shard `shard`'s device views (and the sampler's device actions) as torch tensors, zero
    copy via DLPack: rows are records, as uint8 bytes (rewards: float32 (N, 4)).  They alias the
    engine state, which the engine updates on its own HIP stream (env.stream(shard)): before
    reading them on a torch stream, order that stream after the engine with
    env.signal_stream(stream_handle(), shard) (or runner.sync()); before the engine consumes
    tensors torch wrote, env.wait_stream(stream_handle(), shard) (step_device(ptr) does that
    itself with torch's current stream).  The reference's docs suggest TensorDict over copies of
    the numpy views (docs/source/index.rst:20-26); these need no copy."""
    import torch
    if shard is None:
        if env.num_shards > 1:
            raise ValueError(f"device_tensors of a {env.num_shards}-shard env: pass shard=k "
                             "(each shard's views live on its own GPU)")
        shard = 0
    out = {nm: torch.from_dlpack(env.dlpack(nm, shard)) for nm in DEVICE_VIEWS}
    if sampler is not None:
        out["actions"] = torch.from_dlpack(sampler.dlpack()) if sampler.num_shards == 1 else None
    return out


def stream_handle(device=None):
    """torch's current HIP stream on `device` as an int handle (0 is the null stream, torch's
    default), the stream argument of step_device / wait_stream / signal_stream; None without
    torch."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.current_stream(device).cuda_stream)
    except Exception:
        pass
    return None


def mask_records(envs, source="selected"):
    """A copy of the ActionMask records sample_policy(logits, envs, source) reads, as an (n, 128)
    uint8 torch tensor on the envs' device: "selected", the envs' selected masks, or "stored", each
    env's current agent's stored mask.  A trainer records them before sampling, to evaluate the taken
    actions under new logits later (policy_evaluate).  The copy is taken on torch's current stream,
    after the envs' queued work; single-shard envs only."""
    import torch
    if source not in ("selected", "stored"):
        raise ValueError(f"mask_records: source {source!r} is not 'selected' or 'stored'")
    if envs.num_shards != 1:
        raise ValueError(f"mask_records of a {envs.num_shards}-shard env: it needs a single-shard env (one device)")
    dev = envs.shard_info(0)[2]
    with torch.cuda.device(dev):
        envs.signal_stream(stream_handle(dev), 0)
        if source == "selected":
            return torch.from_dlpack(envs.dlpack("selected_action_masks", 0)).clone()
        obs = torch.from_dlpack(envs.dlpack("observations", 0))             # (n, 17216) ObsData records
        agent = torch.from_dlpack(envs.dlpack("agent_selection", 0)).long() & 3
        # ObsData.player_data[agent].action_mask: byte 16192 + 256 agent + 128 of the record
        cols = (16192 + 128 + 256 * agent)[:, None] + torch.arange(128, device=obs.device)
        return obs.gather(1, cols)


FEATURES_VEC, FEATURES_CHANNELS, FEATURES_MAX_RADIUS = 208, 10, 24


def policy_features(envs, radius=4, *, seat=None, dtype=None, out=None, stream=None):
    """A network's input for every env, seen from one seat: (vec, local), two tensors written by one
    HIP kernel.  The envs' records and views are not touched.

    envs: a single-shard vec env.  radius: an int in [0, 24]; W = 2 radius + 1.  dtype:
    torch.bfloat16 (the default) or torch.float32, for both tensors.  seat: None, the acting seat
    (agent_selection & 3, read on the device); an int 0..3, that seat for every env; or an (n,) uint8
    tensor on the envs' device, one seat per env (its low two bits).  out: None for new tensors, or a
    pair (vec, local) of contiguous tensors of exactly those shapes, that dtype and that device,
    aligned to their element only (slices buf_vec[t], buf_loc[t] of a time-major rollout buffer
    qualify): written in place and returned.

    With s the seat, np the env's n_players, player p's cell (ix_p, iy_p) = (locx - minx + 1,
    locy - miny + 1), the [ix][iy] index of observations.shared.map, and relative seat r = 1..3 the
    player (s + r) mod np when r < np, else absent:
      vec (n, 208), every value as a number (a byte b is float(b), no scaling):
        0 shared.phase; 1..3 shared.current_resources -- the ACTING player's, whatever `seat` says;
        4..21 shared.shop; 22 np; 23, 24 own ix, iy; 25..129 the seat's own DeckObs bytes (draw,
        hand, active, played, discard, 21 types each); 130 + 26 (r - 1) + k for r = 1..3: k = 0
        present, k = 1, 2 ix_r - ix_own, iy_r - iy_own, k = 3 cards in hand, k = 4 cards in draw,
        k = 5..25 per card type the total over the five piles (which pile a card lies in is not
        public); all 26 are 0 for an absent seat.
      local (n, 10, W, W), channel first: entry [c, a, b] is about the map cell (ix_own - radius + a,
        iy_own - radius + b): c = 0..5 map features 1..6 of the cell (shared.map[ix, iy, 1 + c]),
        c = 6, 7, 8: 1 where relative seat 1, 2, 3 stands (players can share a cell), c = 9: 1 where
        the cell lies inside the 48 x 48 grid; a cell outside it has 0 in all ten channels.
    An env with s >= np gets all-zero rows.  float32 values are exact; bfloat16 ones are their round
    to nearest even.  An env whose last reset failed gets unspecified rows.

    The kernel runs on `stream` (default: torch's current stream on the envs' device; -1: the envs'
    own stream) after the envs' queued work, and the envs' later work (the next step overwrites the
    records) runs after it.  Nothing waits on the host.  n == 0 launches nothing."""
    import torch
    who = "policy_features"
    if dtype is None:
        dtype = torch.bfloat16
    if envs.num_shards != 1:
        raise ValueError(f"{who} of a {envs.num_shards}-shard env: it needs a single-shard env (one device)")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= FEATURES_MAX_RADIUS:
        raise ValueError(f"{who}: radius {radius!r} is not an int in [0, {FEATURES_MAX_RADIUS}]")
    if str(dtype) not in _LOGITS_DTYPES:
        raise ValueError(f"{who}: dtype {dtype} is neither torch.float32 nor torch.bfloat16")
    n, dev = envs.num_envs, envs.shard_info(0)[2]
    device = torch.device("cuda", dev)
    w = 2 * radius + 1
    shapes = ((n, FEATURES_VEC), (n, FEATURES_CHANNELS, w, w))
    mode, seat_int, d_seats = 0, 0, 0
    if isinstance(seat, torch.Tensor):
        if seat.device != device or seat.dtype != torch.uint8 or tuple(seat.shape) != (n,) or not seat.is_contiguous():
            raise ValueError(f"{who}: a seats tensor must be a contiguous ({n},) uint8 tensor on {device}, not "
                             f"{tuple(seat.shape)} {seat.dtype} on {seat.device}")
        mode, d_seats = 2, seat.data_ptr()
    elif seat is not None:
        if isinstance(seat, bool) or not isinstance(seat, int) or not 0 <= seat <= 3:
            raise ValueError(f"{who}: seat {seat!r} is not None, an int in 0..3 or an (n,) uint8 tensor")
        mode, seat_int = 1, seat
    if out is None:
        out = tuple(torch.empty(s, dtype=dtype, device=device) for s in shapes)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out):
            raise ValueError(f"{who}: out must be a pair (vec, local) of torch tensors")
        out = tuple(out)
        for name, t, shape in zip(("vec", "local"), out, shapes):
            if tuple(t.shape) != shape:
                raise ValueError(f"{who}: out {name} has shape {tuple(t.shape)}, expected {shape}")
            if t.dtype != dtype:
                raise ValueError(f"{who}: out {name} has dtype {t.dtype}, expected {dtype}")
            if t.device != device:
                raise ValueError(f"{who}: out {name} is on device {t.device}, the envs are on {device}")
            if not t.is_contiguous():
                raise ValueError(f"{who}: out {name} strides {tuple(t.stride())}: it must be contiguous")
    if n == 0:
        return out
    if stream is None:
        stream = stream_handle(dev)
    _C.VecEnvBase.policy_features_raw(envs, radius, _LOGITS_DTYPES[str(dtype)], mode, seat_int, d_seats,
                                      out[0].data_ptr(), out[1].data_ptr(), -1 if stream is None else int(stream))
    return out


_policy_evaluate_fn = None
_LOGITS_DTYPES = {"torch.float32": 0, "torch.bfloat16": 1}


def _policy_evaluate_function():
    """The torch.autograd.Function behind policy_evaluate (built on first use: torch is optional)."""
    global _policy_evaluate_fn
    if _policy_evaluate_fn is not None:
        return _policy_evaluate_fn
    import torch
    from torch.autograd.function import once_differentiable

    def raw(logits, actions, masks, *, logp=None, entropy=None, g_lp=None, g_en=None, grad=None):
        b = logits.shape[0]
        ptr = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
        dev = logits.device.index
        _C.policy_evaluate_raw(b, logits.data_ptr(), _LOGITS_DTYPES[str(logits.dtype)],
                               logits.stride(0) if b > 1 else 92, actions.data_ptr(),
                               actions.stride(0) if b > 1 else actions.shape[1], masks.data_ptr(), ptr(logp),
                               ptr(entropy), ptr(g_lp), ptr(g_en), ptr(grad), dev,
                               int(torch.cuda.current_stream(dev).cuda_stream), grad is not None)

    class PolicyEvaluate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, actions, masks):
            b = logits.shape[0]
            logp = torch.empty(b, dtype=torch.float32, device=logits.device)
            entropy = torch.empty(b, dtype=torch.float32, device=logits.device)
            raw(logits, actions, masks, logp=logp, entropy=entropy)
            ctx.save_for_backward(logits, actions, masks)
            ctx.set_materialize_grads(False)
            return logp, entropy

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lp, g_en):
            logits, actions, masks = ctx.saved_tensors
            g_lp, g_en = (None if g is None else g.to(torch.float32).contiguous() for g in (g_lp, g_en))
            grad = torch.empty((logits.shape[0], 92), dtype=logits.dtype, device=logits.device)
            raw(logits, actions, masks, g_lp=g_lp, g_en=g_en, grad=grad)
            return grad, None, None

    _policy_evaluate_fn = PolicyEvaluate
    return PolicyEvaluate


def policy_evaluate(logits, actions, masks):
    """Joint log-probability of recorded actions and entropy of the five masked categorical heads
    under new logits, differentiable with respect to the logits: the distribution sample_policy
    draws from, for a trainer's update (ratio = exp(policy_evaluate(new_logits, a, m)[0] - old_logp)).
    One HIP kernel forward, one backward, on torch's current stream.

    logits: (B, 92) float32 or bfloat16 on a GPU in ActionMask byte order, stride(1) == 1,
    stride(0) >= 92 (a view such as net_out[:, :92] of a wider layer is taken as is).  actions:
    (B, k) uint8, k >= 5, stride(1) == 1, on the same device: bytes 0..4 of a row are play,
    play_special, remove, move, get_from_shop (the (n, 64) tensor sample_policy returns, a clone of
    it, or its [:, :5] columns in a rollout buffer).  masks: contiguous (B, 128) uint8 ActionMask
    records on the same device (mask_records).  B is any size.  The backward reads the three
    tensors again (nothing else is saved): the sampler's own action tensor, which the next
    sample_policy call overwrites, has to be cloned to outlive that call.

    Returns (logp, entropy), two float32 (B,) tensors.  A head with no valid entry contributes
    nothing.  A row with a +inf logit, or nothing but -inf / NaN, on a non-empty head's valid
    entries, or whose recorded action is not a valid entry, has NaN logp and entropy and an all-zero
    gradient row.  Gradients flow to logits only; double backward is not supported."""
    import torch
    for name, t in (("logits", logits), ("actions", actions), ("masks", masks)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"policy_evaluate: {name} must be a torch tensor")
    if logits.device.type != "cuda":
        raise ValueError(f"policy_evaluate: logits are on device {logits.device}, not on a GPU")
    if logits.dim() != 2 or logits.shape[1] != 92:
        raise ValueError(f"policy_evaluate: logits have shape {tuple(logits.shape)}, expected (B, 92)")
    b = logits.shape[0]
    if str(logits.dtype) not in _LOGITS_DTYPES:
        raise ValueError(f"policy_evaluate: logits dtype {logits.dtype} is neither float32 nor bfloat16")
    if b and (logits.stride(1) != 1 or (b > 1 and logits.stride(0) < 92)):
        raise ValueError(f"policy_evaluate: logits strides {tuple(logits.stride())}: the inner stride must be 1 "
                         "and the row stride at least 92")
    if actions.device != logits.device:
        raise ValueError(f"policy_evaluate: actions are on device {actions.device}, the logits on {logits.device}")
    if actions.dtype != torch.uint8:
        raise ValueError(f"policy_evaluate: actions dtype {actions.dtype} is not uint8")
    if actions.dim() != 2 or actions.shape[0] != b or actions.shape[1] < 5:
        raise ValueError(f"policy_evaluate: actions have shape {tuple(actions.shape)}, expected ({b}, k) with k >= 5")
    if b and (actions.stride(1) != 1 or (b > 1 and actions.stride(0) < 5)):
        raise ValueError(f"policy_evaluate: actions strides {tuple(actions.stride())}: the inner stride must be 1 "
                         "and the row stride at least 5")
    if masks.device != logits.device:
        raise ValueError(f"policy_evaluate: masks are on device {masks.device}, the logits on {logits.device}")
    if masks.dtype != torch.uint8:
        raise ValueError(f"policy_evaluate: masks dtype {masks.dtype} is not uint8")
    if tuple(masks.shape) != (b, 128):
        raise ValueError(f"policy_evaluate: masks have shape {tuple(masks.shape)}, expected ({b}, 128)")
    if not masks.is_contiguous():
        raise ValueError(f"policy_evaluate: masks strides {tuple(masks.stride())}: the records must be contiguous")
    return _policy_evaluate_function().apply(logits, actions, masks)


def turn_gae(values, agents, rewards, dones, last_values=None, *, gamma=0.99, lam=0.95):
    """Per-seat generalised advantage estimation over a time-major window of a turn-based rollout:
    one HIP kernel on torch's current stream, no atomics (the same inputs give the same bits),
    nothing waits on the host.  Returns (advantages, returns), two new contiguous float32 (T, n)
    tensors; there are no gradients (advantages are targets).

    Row t of env i holds the step of seat a = agents[t, i] & 3 (agent_selection BEFORE the step) and
    v = values[t, i], that seat's value estimate there; dones[t, i] and rewards[t, i, :] are the
    env's views AFTER the step.  rewards are read only where dones is set (the engine's rewards view
    is stale between dones: elsewhere it may hold anything, NaN included).  A done of any kind ends
    the episode, and the next row belongs to a new one.  Walking t from T - 1 down to 0 with, per
    seat p, nv[p] = last_values[i, p] (0 when None), A[p] = 0, R[p] = 0:
      1. if dones[t, i]: for all four seats nv[p] = 0, A[p] = 0, R[p] = rewards[t, i, p];
      2. for a only: delta = R[a] + gamma nv[a] - v; A[a] = delta + gamma lam A[a];
         advantages[t, i] = A[a]; returns[t, i] = A[a] + v; nv[a] = v; R[a] = 0.
    gamma discounts per own decision of a seat, not per env row; the terminal reward lands
    undiscounted on each seat's last row of its episode.  last_values[i, p] is seat p's value at the
    state after the last row (a record holds all four players, so a net can give it for any seat).

    values: (T, n) float32 on a GPU, stride(1) == 1, stride(0) >= n (a [:, :n] view of a wider buffer
    is taken as is); agents: (T, n) uint8 and dones: (T, n) uint8 or bool, the same stride rule;
    rewards: (T, n, 4) float32, strides (>= 4 n, 4, 1) with 16-byte aligned rows; last_values:
    contiguous (n, 4) float32 or None; all on one device.  T == 0 or n == 0 launches nothing."""
    import torch
    who = "turn_gae"
    named = [("values", values), ("agents", agents), ("rewards", rewards), ("dones", dones)]
    if last_values is not None:
        named.append(("last_values", last_values))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a torch tensor")
    if values.device.type != "cuda":
        raise ValueError(f"{who}: values are on device {values.device}, not on a GPU")
    if values.dim() != 2:
        raise ValueError(f"{who}: values have shape {tuple(values.shape)}, expected (T, n)")
    T, n = values.shape
    for name, t in named[1:]:
        if t.device != values.device:
            raise ValueError(f"{who}: {name} are on device {t.device}, the values on {values.device}")
    want = {"values": (torch.float32,), "agents": (torch.uint8,), "rewards": (torch.float32,),
            "dones": (torch.uint8, torch.bool), "last_values": (torch.float32,)}
    for name, t in named:
        if t.dtype not in want[name]:
            raise ValueError(f"{who}: {name} dtype {t.dtype} is not " + " or ".join(str(d) for d in want[name]))
    shapes = {"agents": (T, n), "rewards": (T, n, 4), "dones": (T, n), "last_values": (n, 4)}
    for name, t in named[1:]:
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{who}: {name} have shape {tuple(t.shape)}, expected {shapes[name]}")
    out = (torch.empty((T, n), dtype=torch.float32, device=values.device),
           torch.empty((T, n), dtype=torch.float32, device=values.device))
    if T == 0 or n == 0:
        return out
    for name, t in named[:4]:
        inner = 4 if name == "rewards" else 1              # elements per env
        if t.dim() == 3 and t.stride(2) != 1:
            raise ValueError(f"{who}: {name} strides {tuple(t.stride())}: the inner stride must be 1")
        if (n > 1 and t.stride(1) != inner) or (T > 1 and t.stride(0) < inner * n):
            raise ValueError(f"{who}: {name} strides {tuple(t.stride())}: the env stride must be {inner} and the row "
                             f"stride at least {inner * n}")
    rewards_ld = rewards.stride(0) if T > 1 else 4 * n
    if rewards_ld % 4 or rewards.data_ptr() % 16:
        raise ValueError(f"{who}: rewards strides {tuple(rewards.stride())}, storage offset {rewards.storage_offset()}: "
                         "the rows must be 16-byte aligned")
    if last_values is not None and not last_values.is_contiguous():
        raise ValueError(f"{who}: last_values strides {tuple(last_values.stride())}: it must be contiguous")
    ld = lambda t: t.stride(0) if T > 1 else n             # noqa: E731
    dev = values.device.index
    _C.policy_gae_raw(T, n, values.data_ptr(), ld(values), agents.data_ptr(), ld(agents), rewards.data_ptr(), rewards_ld,
                      dones.data_ptr(), ld(dones), 0 if last_values is None else last_values.data_ptr(), float(gamma),
                      float(lam), out[0].data_ptr(), out[1].data_ptr(), dev, int(torch.cuda.current_stream(dev).cuda_stream))
    return out


from .single import cog_env  # noqa: E402  (src/pybind/single_env.cpp: the single-env API)

get_vec_env = _getter(vec.sampler, VEC_ENV_CLS, _make_env_cls)
get_vec_sampler = _getter(vec.env, VEC_SAMPLER_CLS, _make_sampler_cls)
get_runner = _getter(vec.runner, VEC_RUNNER_CLS, _make_runner_cls)
vec.get_vec_env, vec.get_vec_sampler, vec.get_runner = get_vec_env, get_vec_sampler, get_runner

# pre-create the reference's instantiations (vectorized.h:260-267: 0..8, 16, 32, ..., 256)
for _n in list(range(0, 9)) + [16, 32, 64, 128, 256]:
    get_vec_env(_n), get_vec_sampler(_n), get_runner(_n)
del _n, _m

__all__ = ["vec", "Difficulty", "EASY", "MEDIUM", "HARD", "ObsData", "ActionMask", "ActionData", "Info",
           "DeckObs", "SharedObservation", "PlayerData", "PlayerObservation", "action_sampler", "get_vec_env",
           "get_vec_sampler", "get_runner", "device_count", "device_tensors", "stream_handle", "cog_env", "policy_evaluate",
           "mask_records", "turn_gae", "policy_features", "EnvSnapshot"]
