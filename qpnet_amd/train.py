"""Training-side plumbing over the C ABI: autograd.Function for QPNet.forward and a fused
train step (forward + CE + backward + Adam) that never leaves libqpnet_hip for compute.

torch is used for device buffers, streams and the autograd graph only.

One outstanding forward per model: the activations backward needs live in the native handle's
workspace (sized for 288 GB of HBM: whole-chunk activations stay resident), so a second forward of
the same model before the first one's backward would replace them.  Every forward gets a generation
number from the library; a backward whose forward is no longer the current one raises instead of
using the wrong activations."""
import os
import weakref
import collections
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .config import ADAM_FROZEN, ADAM_MAX_GROUPS, adam_group_table


# Walking a module tree for its parameters costs ~0.15 ms of Python per call (120 tensors, 60 sub-modules), and the reference-style
# loop needs the list three times per step.  The list is cached per model and dropped whenever ANY parameter is registered on any module
# (torch's global registration hook: `m.x = nn.Parameter(...)`, `register_parameter`); storages replaced by .to()/.cuda() keep the
# Parameter objects and are caught by ensure_flat's pointer check.
_PARAM_GENERATION = [0]


def _on_parameter_registered(module, name, param):
    _PARAM_GENERATION[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_on_parameter_registered)
# ... and whenever a sub-module is registered (`model.x = other_module` brings parameters without registering any)
torch.nn.modules.module.register_module_module_registration_hook(_on_parameter_registered)


class _AdoptedAdam:
    """What the step hooks keep per stock `torch.optim.Adam` they step themselves (see _adam_prehook)."""
    __slots__ = ("model", "n", "m", "v", "steps", "step_t", "stash", "mviews", "vviews")


_EMPTY = []
_FLAT_OWNERS = weakref.WeakValueDictionary()


def _adam_group_is_plain(g):
    return not (g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable") or g.get("foreach")) \
        and isinstance(g["lr"], float) and g.get("decoupled_weight_decay") in (None, False)


def _adam_adopt(opt):
    """-> _AdoptedAdam when `opt` is a stock Adam with ONE group holding exactly one qpnet_amd module's parameters in order (what
    `torch.optim.Adam(model.parameters(), ...)` builds, reference src/bin/qpnet_train.py:426-429), else None.  The optimizer's state becomes VIEWS of two
    flat moment buffers (a state loaded from a checkpoint is copied into them first), so state_dict() / load_state_dict() keep torch's layout and a
    reference-made checkpoint resumes here and vice versa."""
    if len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    ps = g["params"]
    if not ps or not _adam_group_is_plain(g):
        return None
    model = _FLAT_OWNERS.get(id(ps[0])) if ps[0].__dict__.get("_qpn_flat_view") else None
    if model is None:
        return None
    params = model_params(model)
    flat = getattr(model, "_flat", None)
    if flat is None or not flat.is_cuda or len(params) != len(ps) or any(a is not b for a, b in zip(params, ps)):
        return None
    a = _AdoptedAdam()
    a.model, a.n, a.stash = weakref.ref(model), len(ps), None
    a.m, a.v = torch.zeros_like(flat), torch.zeros_like(flat)
    a.mviews, a.vviews = _split_like(model, a.m), _split_like(model, a.v)
    steps = None
    for p, mv, vv in zip(ps, a.mviews, a.vviews):
        st = opt.state.get(p)
        if not st:
            k = 0
        else:
            if set(st) != {"step", "exp_avg", "exp_avg_sq"}:
                return None
            k = int(float(st["step"]))                    # (a read-back per parameter: once per adoption, i.e. once per optimizer or load_state_dict)
            mv.copy_(st["exp_avg"]); vv.copy_(st["exp_avg_sq"])
        if steps is not None and k != steps:
            return None                                   # parameters stepped a different number of times (some had no gradient): torch's own loop keeps them
        steps = k
    a.steps = steps
    a.step_t = torch.tensor(float(steps), dtype=torch.float32)
    if steps > 0:
        _adam_bind_state(opt, a, ps)
    if not opt.__dict__.get("_qpn_sd_hook"):
        opt.__dict__["_qpn_sd_hook"] = True
        opt.register_state_dict_post_hook(_adam_state_dict_posthook)
    return a


def _adam_state_dict_posthook(opt, sd):
    """state_dict() of an adopted optimizer: every parameter gets a step counter of its OWN (inside the optimizer they all are one host scalar, bumped once
    per step; whoever loads the checkpoint -- torch's own Adam in the reference trainer -- increments them one by one, in place)."""
    a = opt.__dict__.get("_qpn_adopt")
    if a and a.steps > 0:
        sd["state"] = {k: (dict(st, step=torch.tensor(float(a.steps), dtype=torch.float32)) if st.get("step") is a.step_t else st) for k, st in sd["state"].items()}
    return sd


def _adam_bind_state(opt, a, ps):
    for p, mv, vv in zip(ps, a.mviews, a.vviews):
        opt.state[p] = {"step": a.step_t, "exp_avg": mv, "exp_avg_sq": vv}


def _adam_release(opt, a, ps):
    """hand the state back to torch's own implementation (fused=True wants a step counter per parameter, on the device).  Only state the hooks themselves
    own is rewritten -- entries whose step counter IS the adopter's shared host scalar.  A state that `load_state_dict()` has put in their place (a rollback to
    an earlier checkpoint, or an empty state) is left exactly as loaded: its own step counts drive the bias correction from here on, and the next step adopts
    it afresh (the adopter's old count used to overwrite the loaded one, and an empty loaded state got a lone 'step' key)."""
    if a.steps > 0:
        for p in ps:
            st = opt.state.get(p)                         # (.get: the state is a defaultdict -- indexing would create an entry)
            if st and st.get("step") is a.step_t:
                st["step"] = torch.tensor(float(a.steps), dtype=torch.float32, device=p.device)
    opt.__dict__["_qpn_adopt"] = None                     # looked at again at the next step


def _adam_prehook(opt, args, kwargs):
    """The reference trainer builds `torch.optim.Adam(model.parameters(), lr=...)` itself (src/bin/qpnet_train.py:426-429) and steps it once per chunk
    (:531).  With torch's default (foreach) implementation that is ~0.7 ms of host time per step for this model's 120 small tensors, with `fused=True`
    still ~0.25 ms (the per-parameter state walk in Python) -- most of what the unchanged loop spends (tools/dropin_prof.py).  This global step pre-hook
    makes the caller's stock Adam step through the library's ONE Adam kernel over the flat parameter buffer (qpn_adam_step: same update rule, tested
    against torch's, tests/test_train_gpu.py) when that is exactly equivalent:
      * type(opt) is torch.optim.Adam, one group, its parameters = one qpnet_amd module's parameters in order, no amsgrad / maximize / capturable /
        differentiable / foreach / tensor lr, no closure;
      * every p.grad is the view the module's backward handed out (_anchored_backward) -- clipped or rescaled in place is fine; a gradient that was
        replaced is gathered; a missing one (torch skips that parameter) leaves the step to torch.
    The optimizer's state is kept as views of two flat moment buffers (_adam_adopt), the group's hyper-parameters are read every step (lr schedulers
    work unchanged), and while torch's own `step` body runs the group's parameter list is empty, so it does nothing (restored by the post-hook).
    Everything else -- other optimizers, subclasses, several groups -- falls back to `fused=True` on eligible groups or is left alone.
    QPN_DROPIN_FUSED_ADAM=0 switches the hooks off, =torch keeps only the `fused=True` switch."""
    if type(opt) is not torch.optim.Adam:
        return
    d = opt.__dict__
    a = d.get("_qpn_adopt")
    if a is False:
        return
    has_closure = (args[1] if len(args) > 1 else kwargs.get("closure")) is not None       # (args = (optimizer, *step's positional arguments))
    g0 = opt.param_groups[0] if opt.param_groups else None
    if a is not None and a.stash is not None:            # a step that raised between the hooks
        g0["params"] = a.stash; a.stash = None
    if a is None:
        mode = os.environ.get("QPN_DROPIN_FUSED_ADAM", "1")
        if mode == "0":
            d["_qpn_adopt"] = False
            return
        if not d.get("_qpn_checked"):
            d["_qpn_checked"] = True
            _adam_switch_to_fused(opt)
        if mode == "torch" or has_closure:
            return
        try:
            a = _adam_adopt(opt)
        except Exception:                                # (an optimizer state this code does not know: torch's own step, as if the hooks were off)
            a = None
        if a is None:
            d["_qpn_adopt"] = False
            return
        d["_qpn_adopt"] = a
    ps = g0["params"]
    model = a.model()
    if has_closure or len(opt.param_groups) != 1 or model is None or len(ps) != a.n or not _adam_group_is_plain(g0):
        return _adam_release(opt, a, ps)
    flat = getattr(model, "_flat", None)
    if flat is None or flat.numel() != a.m.numel() or flat.device != a.m.device or ps[0].data_ptr() != flat.data_ptr():
        return _adam_release(opt, a, ps)
    c = model.__dict__.get("_qpn_gflat")
    gbuf = None
    if c is not None:
        for p, v in zip(ps, c[2]):
            if p.grad is not v:
                break
        else:
            gbuf = c[1]
    if gbuf is None:
        if any(p.grad is None for p in ps):
            return _adam_release(opt, a, ps)
        gbuf = torch.cat([p.grad.reshape(-1).to(torch.float32) for p in ps])
    if a.steps > 0:
        st = opt.state.get(ps[0]); st1 = opt.state.get(ps[-1])
        if not st or not st1 or st.get("exp_avg") is not a.mviews[0] or st1.get("exp_avg_sq") is not a.vviews[-1] or st["step"] is not a.step_t:
            return _adam_release(opt, a, ps)              # load_state_dict() replaced the state: adopted again at the next step
    dev = flat.device
    L, hd = model._native(dev)
    b1, b2 = g0["betas"]
    with torch.cuda.device(dev):
        _lib.check(L.qpn_train_status_collect(hd))       # a pending forward check (no-op after a backward has collected it)
        _groups_off(model, L, hd)                        # (a grouped FusedTrainer / FlatAdam may have stepped this module before: this optimizer has ONE group over everything)
        _lib.check(L.qpn_adam_step(hd, flat.data_ptr(), gbuf.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), flat.numel(), a.steps + 1,
                                   g0["lr"], b1, b2, g0["eps"], g0["weight_decay"], torch.cuda.current_stream(dev).cuda_stream))
    a.steps += 1
    a.step_t += 1
    if a.steps == 1:
        _adam_bind_state(opt, a, ps)
    a.stash = ps
    g0["params"] = _EMPTY


def _adam_posthook(opt, args, kwargs):
    a = opt.__dict__.get("_qpn_adopt")
    if a and a.stash is not None:
        opt.param_groups[0]["params"] = a.stash
        a.stash = None


def _adam_switch_to_fused(opt):
    """eligible groups of a stock Adam -> torch's own fused implementation (what runs whenever _adam_prehook leaves a step to torch)."""
    for g in opt.param_groups:
        ps = g["params"]
        if not ps or g.get("fused") is not None or g.get("foreach") is not None or g.get("capturable") or g.get("differentiable") or g.get("amsgrad"):
            continue
        if not all(p.__dict__.get("_qpn_flat_view") and p.is_cuda and p.dtype == torch.float32 for p in ps):
            continue
        g["fused"] = True
        for p in ps:                                  # a state loaded from a checkpoint keeps its step counters on the host: the fused kernel wants them next to the parameter
            st = opt.state.get(p)
            if st and "step" in st and torch.is_tensor(st["step"]) and st["step"].device != p.device:
                st["step"] = st["step"].to(device=p.device, dtype=torch.float32)


from torch.optim.optimizer import register_optimizer_step_pre_hook as _register_optimizer_step_pre_hook  # noqa: E402
from torch.optim.optimizer import register_optimizer_step_post_hook as _register_optimizer_step_post_hook  # noqa: E402
_register_optimizer_step_pre_hook(_adam_prehook)
_register_optimizer_step_post_hook(_adam_posthook)


def join_staged(x, dev, *more):
    """Inputs copied to the device on a stream of their own (runners.PinnedStager: the copy must not sit between the step's kernels on the compute stream) carry
    {ready event, device buffer}: the consumer's stream waits for the copy -- long done when a prefetch thread is ahead, so the wait is a queue packet, not a
    stall -- and the buffer is marked as used on that stream (the caching allocator will not hand it out again before the step that reads it has run).
    Every consumer of loader batches calls this on ALL its inputs (FusedTrainer.step / forward_loss, QPNet.forward): a tensor that never
    went through a stager costs one dictionary look-up."""
    done = None
    for t in (x,) + more:
        st = t.__dict__.get("_qpn_staged") if isinstance(t, torch.Tensor) else None
        if st is None:
            continue
        if st[0] is not done:                          # (the tensors of one batch share one copy: one wait, one record_stream)
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(st[0])
            st[1].record_stream(cur)
            done = st[0]
        del t.__dict__["_qpn_staged"]                  # (once per batch)


def model_params(model):
    """list(model.parameters()), cached (see above)."""
    c = model.__dict__.get("_qpn_params")
    # (deletions -- `del model.x` -- fire no hook: the count of registered sub-modules / parameters of the top level is part of the key)
    key = (_PARAM_GENERATION[0], len(model._modules), len(model._parameters))
    if c is None or c[0] != key:
        c = (key, list(model.parameters()))
        model.__dict__["_qpn_params"] = c
    return c[1]


def ensure_flat(model, dev):
    """One contiguous fp32 buffer holding every parameter in state_dict order, with the
    nn.Parameters re-pointed at views of it (so optimizers / load_state_dict write into it and
    the C ABI reads it without a gather).  Rebuilt if .to()/.cuda() replaced the storages."""
    params = model_params(model)
    flat = getattr(model, "_flat", None)
    ok = flat is not None and flat.device == dev
    if ok:
        # 120 data_ptr() calls cost ~60 us of interpreter time per step: the full walk runs when the parameter list was rebuilt and every 32nd call; every
        # call looks at the first and the last view (.to() / .cuda() / load into new storage replace ALL of them) and at FOUR more in rotation, with their
        # dtype -- a single interior `p.data = ...` (pruning, re-parametrisation, a partial load with assign=True) is seen within 30 calls at the latest
        c = model.__dict__.get("_qpn_flat_chk")
        base = flat.data_ptr()
        if c is not None and c[0] is params and c[1] < 32:
            c[1] += 1
            last = params[-1]
            ok = params[0].data_ptr() == base and last.data_ptr() == base + 4 * (flat.numel() - last.numel()) and last.dtype == torch.float32
            offs, k, n = c[2], c[3], len(params)
            for _ in range(4):
                k = k + 1 if k + 1 < n else 0
                q = params[k]
                if q.data_ptr() != base + 4 * offs[k] or q.dtype != torch.float32:
                    ok = False
            c[3] = k
        else:
            o, offs = 0, []
            for p in params:
                if p.data_ptr() != base + 4 * o or p.dtype != torch.float32:
                    ok = False
                    break
                offs.append(o)
                o += p.numel()
            model.__dict__["_qpn_flat_chk"] = [params, 0, offs, 0] if ok else None
    if not ok:
        flat = torch.cat([p.detach().reshape(-1).to(dev, torch.float32) for p in params]).contiguous()
        o = 0
        _FLAT_OWNERS[id(params[0])] = model             # (looked up by _adam_adopt, which checks every parameter's identity against this module's)
        for p in params:
            n = p.numel()
            p.data = flat[o:o + n].view(p.shape)
            p.__dict__["_qpn_flat_view"] = True      # (what _adam_prehook recognises this module's parameters by; a plain bool: parameters get pickled)
            o += n
        model._flat = flat
    return model._flat


def _split_like(model, gflat):
    """views of the flat gradient, one per parameter: ONE split call + a reshape for the tensors that are not 1-D (slicing and viewing
    each of the 120 by hand was 0.27 ms of the backward's host time)."""
    params = model_params(model)
    c = model.__dict__.get("_qpn_split")
    if c is None or c[0] is not params:
        c = (params, [p.numel() for p in params], [tuple(p.shape) if p.dim() != 1 else None for p in params])
        model.__dict__["_qpn_split"] = c
    pieces = gflat.split_with_sizes(c[1])
    return [g if shp is None else g.view(shp) for g, shp in zip(pieces, c[2])]


def _flat_grad_of(params):
    """The flat gradient buffer the parameters' .grad tensors are consecutive views of, or None."""
    if not params or params[0].grad is None:
        return None
    base = params[0].grad.data_ptr()
    o = 0
    for p in params:
        g = p.grad
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.data_ptr() != base + 4 * o:
            return None
        o += p.numel()
    g0 = params[0].grad
    return torch.as_strided(g0, (o,), (1,), g0.storage_offset()) if g0.untyped_storage().nbytes() >= 4 * (g0.storage_offset() + o) else None


def _arm_input_grad(L, hd, dh):
    """the next backward on this handle also writes dL/dh into `dh` (qpn_train_input_grad: one shot); None: nothing to arm"""
    if dh is not None:
        _lib.check(L.qpn_train_input_grad(hd, dh.data_ptr(), dh.numel()))


class QPNetFunction(torch.autograd.Function):
    """logits = QPNet.forward(x, h, d, blength); backward = hand-written HIP kernels.
    Gradients: the parameters, and the auxiliary features `h` when they require one (the same backward writes it: there is no input-only backward -- with every
    parameter frozen the weight gradients are still computed, into a scratch buffer).  `dilated_factors` gets None: the pitch tap is a rounding of the factor, its
    derivative is zero almost everywhere -- what the reference's autograd yields there too.  Once differentiable: the backward is not itself recorded."""

    @staticmethod
    def forward(ctx, model, x, h, d, BL, maxd, *params):
        dev = x.device
        L, hd = model._native(dev)
        flat = model._flat                                    # (qpnet_forward has just validated it)
        B, T = x.shape
        logits = torch.empty((B, BL, model.n_quantize), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            # The reference asserts on the gather bounds inside forward (qpnet.py:294).  Here the device-side check is enqueued behind
            # the kernels and collected (no stream drain) at the first of: this forward's backward (so an out-of-range factor is raised
            # BEFORE the optimizer step it would feed), FlatAdam.step, the next forward, model.check_status().  A forward that records no
            # graph (torch.no_grad() / eval loops: nothing else of this model may ever run) checks synchronously.
            _lib.check(L.qpn_train_status_collect(hd))
            _lib.check(L.qpn_train_forward(hd, flat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd,
                                           x.data_ptr(), h.data_ptr(), d.data_ptr(), logits.data_ptr(), stream))
            if model._qpn_sync_status:
                _lib.check(L.qpn_train_status(hd, stream))
            else:
                _lib.check(L.qpn_train_status_enqueue(hd, stream))
        ctx.model = model
        ctx.anchored = len(params) == 1 and params[0] is model.__dict__.get("_qpn_anchor")
        ctx.generation = int(L.qpn_train_generation(hd))
        ctx.keep = (x, h, d)                                  # inputs must outlive backward (the workspace points into them)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits):
        model = ctx.model
        dev = dlogits.device
        L, hd = model._native(dev)
        if int(L.qpn_train_generation(hd)) != ctx.generation:
            raise RuntimeError("qpnet_amd: backward of a forward whose activations have been replaced by a later forward of the "
                               "same model (one outstanding forward per model; run validation forwards after backward)")
        with torch.cuda.device(dev):
            # the forward's gather-bounds / target check.  Default: WAIT for its copy (it sits behind the forward's kernels, so a host that runs ahead of
            # the device blocks here until the forward has drained) -- the one way to raise BEFORE an optimizer this module does not control (stock
            # torch.optim.Adam) steps on a flagged gradient, as the reference's in-line assert does (qpnet.py:294).  model.status_check = "lazy": only
            # what has already landed is looked at (hipEventQuery); the rest is collected by FlatAdam.step / the next forward / model.check_status(),
            # and the fused Adam kernel skips flagged updates on the device by itself.
            if getattr(model, "status_check", "backward") == "lazy":
                _lib.check(L.qpn_train_status_poll(hd, None))
            else:
                _lib.check(L.qpn_train_status_collect(hd))
        flat = model._flat
        dl = dlogits.contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        # the features' gradient (h.requires_grad): a fresh buffer the backward's own launches fill, every element (qpn_train_input_grad)
        dh = torch.empty_like(ctx.keep[1]) if ctx.needs_input_grad[2] else None
        if ctx.anchored:
            _anchored_backward(model, L, hd, dl, flat, stream, dev, dh)
            return (None, None, dh, None, None, None, None)
        # a FRESH buffer per backward: autograd keeps (or accumulates into) the views it is handed, so they must not
        # alias memory a later backward writes (only the features want a gradient: the buffer is scratch)
        g = torch.empty_like(flat)
        with torch.cuda.device(dev):
            _arm_input_grad(L, hd, dh)
            _lib.check(L.qpn_train_backward(hd, dl.data_ptr(), g.data_ptr(), stream))
        return (None, None, dh, None, None, None) + tuple(v if need else None for v, need in zip(_split_like(model, g), ctx.needs_input_grad[6:]))


def _anchored_backward(model, L, hd, dl, flat, stream, dev, dh=None):
    """The reference loop's backward without autograd's 120-way fan-out (qpnet_train.py:527-531: zero_grad, loss.backward(), optimizer.step()).
    The graph holds ONE anchor leaf instead of the 120 parameters, and this function gives every parameter its .grad itself, with
    loss.backward()'s semantics: parameters without a gradient (after optimizer.zero_grad(), whose default sets them to None) get one, the
    others accumulate.  The gradients are consecutive views of one persistent flat buffer the kernels write directly (NOTE the aliasing: a reference
    to a p.grad kept across zero_grad(set_to_none=True) is overwritten by the next backward, unlike torch's fresh tensors), so the usual step
    costs one launch sequence and 120 attribute stores -- measured on the host: 0.63 -> 0.25 ms of the 1.63 ms the unchanged loop spends per step
    (autograd built 120 views and ran 120 AccumulateGrad nodes).  Not visible to this path: torch.autograd.grad() w.r.t. parameters (torch
    reports them as unused in the graph) and tensor hooks on parameters; QPN_DROPIN_FLAT_GRAD=0 hands autograd the parameters as before."""
    params = model_params(model)
    c = model.__dict__.get("_qpn_gflat")
    if c is None or c[0] is not params or c[1].device != dev or c[1].numel() != flat.numel():
        g = torch.zeros_like(flat)
        c = (params, g, _split_like(model, g))
        model.__dict__["_qpn_gflat"] = c
    gflat, views = c[1], c[2]
    none_yet = params[0].grad is None and all(p.grad is None for p in params)
    mine = False
    if not none_yet:
        fb = _flat_grad_of(params)
        mine = fb is not None and fb.data_ptr() == gflat.data_ptr()
    with torch.cuda.device(dev):
        _arm_input_grad(L, hd, dh)                         # (consumed by whichever of the two backward calls below runs)
        if none_yet:                                       # the usual step: the kernels write the buffer the .grad views live in
            _lib.check(L.qpn_train_backward(hd, dl.data_ptr(), gflat.data_ptr(), stream))
            for p, v in zip(params, views):
                p.grad = v
            return
        tmp = torch.empty_like(flat)
        _lib.check(L.qpn_train_backward(hd, dl.data_ptr(), tmp.data_ptr(), stream))
    if mine:                                               # accumulation (two backwards, or zero_grad(set_to_none=False)): one add
        gflat.add_(tmp)
        return
    for p, v, t in zip(params, views, _split_like(model, tmp)):      # somebody replaced some of the gradients: one by one
        if p.grad is None:
            v.copy_(t); p.grad = v
        else:
            p.grad.add_(t)


def forward_maxd(model, T, F, Td, BL, dilated_factors):
    """ceil(max d) as QPNet.forward needs it (reference qpnet.py:254-262: it sets the receptive field RF = RF_A * maxd +
    RF_F + 1 and the chunk's last RF + BL samples are used) WITHOUT reading the factors back from the device.

    The largest maxd the chunk's shapes admit is used instead: RF_A * maxd + RF_F + 1 + BL <= min(T, Td + 1, F * U + 1).  Any
    maxd >= the true ceil(max d) gives the same logits -- the extra leading rows are context the last BL outputs do not see,
    and the pitch taps are positions counted from the END of the chunk -- while a true maximum that does NOT fit the chunk
    is what the reference's gather assert (qpnet.py:294) catches; here the device-side bound check reports it.  The
    reference trainer cuts chunks of exactly RF + BL samples (qpnet_train.py:268-284), for which this IS ceil(max d).
    `model.read_back_maxd = True` restores the device read-back (one stream synchronisation per forward)."""
    recA, recF = model.receptiveA_field, model.receptiveF_field
    if getattr(model, "read_back_maxd", False) or recA <= 0:
        return int(torch.max(dilated_factors.ceil()))
    U = model.upsampling_factor
    avail = min(int(T), int(Td) + 1, (int(F) * U if U > 0 else int(F)) + 1)
    return max((avail - recF - 1 - int(BL)) // recA, 1)


def qpnet_forward(model, x, h, dilated_factors, blength):
    """QPNet.forward (reference qpnet.py:239-262 for the argument handling)."""
    dev = x.device
    if dev.type != "cuda":
        raise RuntimeError("qpnet_amd.QPNet runs on an AMD GPU only (tensors are on %s); there is no CPU fallback" % dev)
    # (one read-back when blength lives on the device, as in the reference trainer; a host tensor / array costs nothing)
    bl_host = blength.tolist() if hasattr(blength, "tolist") else list(blength)
    assert all(v == bl_host[0] for v in bl_host)
    BL = int(bl_host[0])
    join_staged(x, dev, h, dilated_factors)
    maxd = forward_maxd(model, x.shape[1], h.shape[2], dilated_factors.shape[1], BL, dilated_factors)
    x = x.to(dev, torch.int64).contiguous()
    h = h.to(dev, torch.float32).contiguous()
    d = dilated_factors.to(dev, torch.float32).contiguous()
    ensure_flat(model, dev)
    params = model_params(model)
    # no graph will be recorded (no_grad, or neither a parameter nor the features want a gradient): no backward will come to collect the status
    wants = [p.requires_grad for p in params]
    model._qpn_sync_status = not (torch.is_grad_enabled() and (any(wants) or h.requires_grad))
    if torch.is_grad_enabled() and all(wants) and os.environ.get("QPN_DROPIN_FLAT_GRAD", "1") != "0":
        # every parameter trains (the reference trainer): ONE anchor leaf stands for them in the graph, the backward assigns their gradients (_anchored_backward)
        a = model.__dict__.get("_qpn_anchor")
        if a is None or a.device != dev:
            a = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)
            model.__dict__["_qpn_anchor"] = a
        return QPNetFunction.apply(model, x, h, d, BL, maxd, a)
    return QPNetFunction.apply(model, x, h, d, BL, maxd, *params)


Score = collections.namedtuple("Score", "nll entropy argmax rank")
Score.__doc__ = """Per-sample records of score_logits, each (B, BL): nll (float32, nats; +inf where the target is outside [0, n_quantize)), entropy (float32, nats),
argmax (int32, the lowest index among the maxima), rank (int32, the number of classes whose logit is strictly above the target's; n_quantize for a
target out of range).  top-k accuracy is (rank < k); nll.double().mean() is the cross entropy the library reports for the same rows."""


def score_logits(logits, targets):
    """Teacher-forced scoring of given logits (qpn_score_logits): logits (B, BL, Q) float32 on the GPU, targets (B, >= BL) int64 whose LAST BL columns are
    scored (batch_t[:, -batch_length:], as the loss takes them) -> Score.  The four tensors are views of one (B, BL) buffer of 16-byte records.  Runs on
    the current stream and does not synchronise; nothing here is differentiable."""
    dev = logits.device
    if dev.type != "cuda" or targets.device.type != "cuda":
        raise RuntimeError("qpnet_amd.score_logits runs on an AMD GPU only (tensors are on %s / %s); there is no CPU fallback" % (dev, targets.device))
    if logits.dim() != 3 or targets.dim() != 2 or targets.shape[0] != logits.shape[0]:
        raise ValueError("score_logits: logits (B, BL, Q) and targets (B, >= BL) expected, got %s and %s" % (tuple(logits.shape), tuple(targets.shape)))
    lg = logits.detach().to(dev, torch.float32).contiguous()
    tg = targets.to(dev, torch.int64).contiguous()
    B, BL, Q = lg.shape
    rec = torch.empty((B, BL, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qpn_score_logits(lg.data_ptr(), tg.data_ptr(), tg.shape[1], B, BL, Q, rec.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    ints = rec.view(torch.int32)
    return Score(rec[..., 0], rec[..., 1], ints[..., 2], ints[..., 3])


def _check_max_grad_norm(v):
    """max_grad_norm as the C ABI takes it: None / 0 -> 0.0 (clipping off); a negative or non-finite value raises."""
    if v is None:
        return 0.0
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError("max_grad_norm must be a finite number >= 0 (None or 0: no clipping), got %r" % (v,))
    return v


def _check_ema_decay(v):
    """ema_decay as the C ABI takes it: None / 0 -> 0.0 (no averaged weights); otherwise it must lie in (0, 1) as an fp32 number too (the kernel's factor is
    float32(1) - float32(decay))."""
    if v is None:
        return 0.0
    v = float(v)
    if v == 0.0:
        return 0.0
    if not (0.0 < v < 1.0) or not (0.0 < float(np.float32(v)) < 1.0):
        raise ValueError("ema_decay must lie in (0, 1) (None or 0: no averaged weights), got %r" % (v,))
    return v


def _check_h_grad(h_grad, h, dev):
    """FusedTrainer.step's h_grad as the C ABI takes it: float32, shaped like h, contiguous, on the (CUDA) device of the step's inputs."""
    if not isinstance(h_grad, torch.Tensor):
        raise ValueError("h_grad must be a torch.Tensor (or None), got %r" % (type(h_grad),))
    if h_grad.dtype != torch.float32:
        raise ValueError("h_grad must be float32, got %s" % (h_grad.dtype,))
    if tuple(h_grad.shape) != tuple(h.shape):
        raise ValueError("h_grad must be shaped like h %s, got %s" % (tuple(h.shape), tuple(h_grad.shape)))
    if not h_grad.is_contiguous():
        raise ValueError("h_grad must be contiguous")
    if not h_grad.is_cuda or h_grad.device != dev:
        raise ValueError("h_grad must be a CUDA tensor on the device of the step's inputs (%s), got %s" % (dev, h_grad.device))


def _check_distill_scalars(alpha, temperature):
    """alpha / temperature of the soft-target loss as the C ABI takes them (qpn_train_distill's rules, after rounding to float32): alpha in (0, 1],
    temperature finite and > 0 -> (float, float)"""
    try:
        with np.errstate(over="ignore"):                   # (a value beyond float32 rounds to inf, which the rules below refuse)
            a, T = float(np.float32(alpha)), float(np.float32(temperature))
    except (TypeError, ValueError):
        raise ValueError("distill: alpha and temperature must be numbers, got %r and %r" % (alpha, temperature))
    if not (0.0 < a <= 1.0):
        raise ValueError("distill: alpha must lie in (0, 1] as a float32 number, got %r" % (alpha,))
    if not (T > 0.0) or not np.isfinite(T):
        raise ValueError("distill: temperature must be finite and > 0 as a float32 number, got %r" % (temperature,))
    return a, T


def check_distill_geometry(student, teacher):
    """the two models of a distillation must agree where their inputs and their logits meet: n_quantize, n_aux and upsampling_factor (anything with these three
    attributes: modules or configurations); raises ValueError naming the first that differs"""
    for k in ("n_quantize", "n_aux", "upsampling_factor"):
        if getattr(student, k) != getattr(teacher, k):
            raise ValueError("distill: teacher and student differ in %s (%r against %r)" % (k, getattr(teacher, k), getattr(student, k)))


def _check_distill(model, distill):
    """FusedTrainer's distill= -> None, or (teacher or None, alpha, temperature); every error is a ValueError, raised before any device work"""
    if distill is None:
        return None
    if not isinstance(distill, dict):
        raise ValueError('distill must be None or a dict {"teacher": QPNet, "alpha": a, "temperature": T}, got %r' % (type(distill),))
    unknown = sorted(set(distill) - {"teacher", "alpha", "temperature"})
    if unknown:
        raise ValueError("distill: unknown keys %s" % (unknown,))
    if "alpha" not in distill or "temperature" not in distill:
        raise ValueError('distill needs "alpha" and "temperature"')
    a, T = _check_distill_scalars(distill["alpha"], distill["temperature"])
    teacher = distill.get("teacher")
    if teacher is not None:
        if teacher is model:
            raise ValueError("distill: the teacher is the student itself (one outstanding forward per model)")
        if not all(hasattr(teacher, k) for k in ("n_quantize", "n_aux", "upsampling_factor", "_native")):
            raise ValueError("distill: the teacher must be a qpnet_amd.QPNet, got %r" % (type(teacher),))
        check_distill_geometry(model, teacher)
    return teacher, a, T


def _check_step_tensor(name, label, v, shape, dev):
    """a step's precomputed teacher logits or sample weights as the C ABI takes them: float32, `shape` (named `label` in the message), contiguous, on the (CUDA)
    device of the step's inputs"""
    if not isinstance(v, torch.Tensor):
        raise ValueError("%s must be a torch.Tensor (or None), got %r" % (name, type(v)))
    if v.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, v.dtype))
    if tuple(v.shape) != shape:
        raise ValueError("%s must have the shape %s = %s, got %s" % (name, label, shape, tuple(v.shape)))
    if not v.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if not v.is_cuda or v.device != dev:
        raise ValueError("%s must be a CUDA tensor on the device of the step's inputs (%s), got %s" % (name, dev, v.device))


_LOSS_HANDLES = {}


def _loss_handle(dev, Q):
    """a native handle per (device, n_quantize) for the loss calls that take their class count from a handle and nothing else (qpn_distill_loss)"""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), Q)
    hp = _LOSS_HANDLES.get(key)
    if hp is None:
        import dataclasses
        from .config import TINY
        hp = C.c_void_p()
        _lib.check(_lib.lib().qpn_create(C.byref(_lib.make_config(dataclasses.replace(TINY, n_quantize=Q))), C.byref(hp)))
        _LOSS_HANDLES[key] = hp
    return hp


def distill_loss(logits, teacher_logits, targets, alpha, temperature, sample_weights=None, ignore_index=None):
    """The soft-target loss of the fused step for a reference-style loop (qpn_distill_loss): logits, teacher_logits (B, BL, Q) float32 on the GPU, targets
    (B, >= BL) int64 whose LAST BL columns are the hard targets ->  mean over rows of (1 - alpha) CE(z, y) + alpha T^2 KL(softmax(t / T) || softmax(z / T)),
    a float32 scalar whose backward hands grad_output * dL/dlogits (computed by the same kernel launch) to `logits` only.  Once differentiable.  Reads the loss in the
    call (one stream drain, as the reference's loss.item()); a NaN or an infinity in teacher_logits raises QpnError(-4).
    sample_weights (B, BL) / ignore_index: the row weights of cross_entropy() below (qpn_distill_loss_opts): w_r multiplies the whole row loss, CE and KL term
    alike, over the row count."""
    ign, _, _ = _check_loss_options(ignore_index, 0.0, "rows")
    if sample_weights is not None:
        _check_weights_like(sample_weights, logits.shape[0] * logits.shape[1] if logits.dim() == 3 else -1)
    dev = logits.device
    if dev.type != "cuda" or teacher_logits.device != dev or targets.device.type != "cuda":
        raise RuntimeError("qpnet_amd.distill_loss runs on an AMD GPU only (tensors are on %s / %s / %s); there is no CPU fallback" % (dev, teacher_logits.device, targets.device))
    if logits.dim() != 3 or tuple(teacher_logits.shape) != tuple(logits.shape) or targets.dim() != 2 or targets.shape[0] != logits.shape[0] or targets.shape[1] < logits.shape[1]:
        raise ValueError("distill_loss: logits and teacher_logits (B, BL, Q) and targets (B, >= BL) expected, got %s, %s and %s"
                         % (tuple(logits.shape), tuple(teacher_logits.shape), tuple(targets.shape)))
    a, T = _check_distill_scalars(alpha, temperature)
    return _NativeLoss.apply(logits, targets, teacher_logits, a, T, sample_weights, ign, 0.0, 0)


_LOSS_NORMS = {"rows": 0, "weights": 1}


def _check_loss_options(ignore_index, label_smoothing, norm):
    """the loss options as the C ABI takes them (qpn_loss_opts' rules, eps after rounding to float32) -> (ignore_index or None, eps, norm code); every error is a
    ValueError"""
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)) or not -2 ** 63 <= int(ignore_index) < 2 ** 63):
        raise ValueError("ignore_index must be None or an int (a 64-bit one), got %r" % (ignore_index,))
    try:
        eps = float("nan") if isinstance(label_smoothing, (bool, str, bytes)) or label_smoothing is None else float(np.float32(label_smoothing))
    except (TypeError, ValueError):
        raise ValueError("label_smoothing must be a number, got %r" % (label_smoothing,))
    if not (0.0 <= eps < 1.0):
        raise ValueError("label_smoothing must lie in [0, 1) as a float32 number, got %r" % (label_smoothing,))
    if not isinstance(norm, str) or norm not in _LOSS_NORMS:
        raise ValueError('norm must be "rows" (divide by the row count) or "weights" (divide by the sum of the weights), got %r' % (norm,))
    return (None if ignore_index is None else int(ignore_index)), eps, _LOSS_NORMS[norm]


def _check_weights_like(w, rows):
    if not isinstance(w, torch.Tensor):
        raise ValueError("sample_weights must be a torch.Tensor (or None), got %r" % (type(w),))
    if not w.is_floating_point():
        raise ValueError("sample_weights must be a floating-point tensor, got %s" % (w.dtype,))
    if w.numel() != rows:
        raise ValueError("sample_weights must hold one weight per row (%d), got the shape %s" % (rows, tuple(w.shape)))


def _make_loss_opts(weights, ignore_index, eps, norm):
    """qpn_loss_opts from checked values (weights: a float32 contiguous CUDA tensor or None, kept alive by the caller)"""
    return _lib.QpnLossOpts(weights.data_ptr() if weights is not None else None, weights.numel() if weights is not None else 0,
                            0 if ignore_index is None else 1, 0 if ignore_index is None else ignore_index, eps, norm)


class _NativeLoss(torch.autograd.Function):
    """cross_entropy() (teacher_logits None) and distill_loss(): one launch computes the loss and dL/dlogits, backward scales the saved dL/dlogits"""
    @staticmethod
    def forward(ctx, logits, targets, teacher_logits, alpha, temperature, weights, ignore, eps, norm):
        dev = logits.device
        lg = logits.detach().to(dev, torch.float32).contiguous()
        tg = targets.to(dev, torch.int64).contiguous()
        if lg.dim() == 2:                                   # (rows, Q) and (rows,): the reference's criterion(output.view(-1, Q), t.view(-1))
            lg, tg = lg[None], tg[None]
        B, BL, Q = lg.shape
        wt = None if weights is None else weights.detach().to(dev, torch.float32).contiguous()
        dl = torch.empty_like(lg)
        parts = (C.c_double * 4)()
        opts = _make_loss_opts(wt, ignore, eps, norm)
        L = _lib.lib()
        with torch.cuda.device(dev):
            hp = _loss_handle(dev, Q)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if teacher_logits is None:
                rc = L.qpn_ce_loss_opts(hp, lg.data_ptr(), tg.data_ptr(), tg.shape[1], B, BL, C.byref(opts), dl.data_ptr(), parts, stream)
            else:
                tl = teacher_logits.detach().to(dev, torch.float32).contiguous()
                head = (hp, lg.data_ptr(), tl.data_ptr(), tg.data_ptr(), tg.shape[1], B, BL, alpha, temperature)
                if weights is None and ignore is None:      # the entry point without options: its kernels are instances of their own
                    rc = L.qpn_distill_loss(*head, dl.data_ptr(), parts, stream)
                else:
                    rc = L.qpn_distill_loss_opts(*head, C.byref(opts), dl.data_ptr(), parts, stream)
            _lib.check(rc)
            _lib.check(L.qpn_train_status(hp, stream))      # (the stream has just been drained for the loss)
        ctx.save_for_backward(dl.view(logits.shape))
        return torch.tensor(parts[0], dtype=torch.float32, device=dev)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        dl, = ctx.saved_tensors
        return (grad_output * dl,) + (None,) * 8


def cross_entropy(logits, targets, sample_weights=None, ignore_index=None, label_smoothing=0.0, norm="rows"):
    """The fused step's criterion with its options for a reference-style loop (qpn_ce_loss_opts; DESIGN.md section 5, "Loss options") -- a drop-in for
    `criterion = torch.nn.CrossEntropyLoss()`: logits (B, BL, Q) float32 on the GPU with targets (B, >= BL) int64 whose LAST BL columns are the targets, or the
    reference's flattened pair, logits (rows, Q) and targets (rows,).  With w_r = sample_weights[r] (one per row; 1 without), 0 where the target equals ignore_index:
        L = (1 / N) sum_r w_r (lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q),   N = the row count (norm="rows") or sum_r w_r (norm="weights": torch's mean with
    ignore_index), a float32 scalar whose backward hands grad_output * dL/dlogits (computed by the same kernel launch) to `logits` only.  Once differentiable.  Rows
    of weight 0 are not read (their targets may hold anything).  Reads the loss in the call (one stream drain, as the reference's loss.item()); a NaN, infinite or
    negative weight raises QpnError(-4), as a target outside [0, Q) in a live row does.  No CPU fallback; argument errors are ValueErrors before any device work."""
    if not isinstance(logits, torch.Tensor) or not isinstance(targets, torch.Tensor):
        raise ValueError("cross_entropy: logits and targets must be torch.Tensors")
    flat = logits.dim() == 2
    if flat:
        ok = targets.dim() == 1 and targets.shape[0] == logits.shape[0]
    else:
        ok = logits.dim() == 3 and targets.dim() == 2 and targets.shape[0] == logits.shape[0] and targets.shape[1] >= logits.shape[1]
    if not ok or logits.numel() == 0:
        raise ValueError("cross_entropy: logits (B, BL, Q) and targets (B, >= BL), or logits (rows, Q) and targets (rows,), expected, got %s and %s"
                         % (tuple(logits.shape), tuple(targets.shape)))
    ign, eps, code = _check_loss_options(ignore_index, label_smoothing, norm)
    if sample_weights is not None:
        _check_weights_like(sample_weights, logits.numel() // logits.shape[-1])
    dev = logits.device
    if dev.type != "cuda" or targets.device.type != "cuda" or (sample_weights is not None and sample_weights.device.type != "cuda"):
        raise ValueError("qpnet_amd.train.cross_entropy runs on an AMD GPU only (logits are on %s, targets on %s); there is no CPU fallback" % (dev, targets.device))
    return _NativeLoss.apply(logits, targets, None, 0.0, 0.0, sample_weights, ign, eps, code)


def _check_accum_steps(v):
    """accum_steps as the C ABI's micro_count: a plain int >= 1 (a bool, a float or None is not one)."""
    if type(v) is not int or v < 1:
        raise ValueError("accum_steps must be an int >= 1 (1: one update per chunk), got %r" % (v,))
    return v


# ---------------------------------------------------------------- averaged weights (EMA) shared by FusedTrainer and FlatAdam
def _ema_home(ema, flat):
    """the averaged weights next to `flat`: a copy of the weights the first time (or after load_ema(None)), re-homed like the moments when the device changed."""
    if ema is None or ema.numel() != flat.numel():
        return flat.detach().clone()
    if ema.device != flat.device:
        return ema.to(flat.device)
    return ema


def _ema_to_state_dict(model, ema):
    """the flat average under the model's state_dict() keys, shapes and order (copies: the buffer goes on moving)."""
    if ema is None:                                  # averaging on, no step yet: the average of nothing but the seed is the weights
        return collections.OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())
    return collections.OrderedDict(zip(model.state_dict().keys(), (t.clone() for t in _split_like(model, ema))))


def _ema_from_state_dict(model, sd):
    """inverse of _ema_to_state_dict: one flat fp32 tensor on the model's device (a CPU model: moved at the first step, as the moments are)."""
    ref = model.state_dict()
    if list(sd.keys()) != list(ref.keys()):
        raise ValueError("averaged weights: the keys differ from the model's state_dict()")
    for k, v in ref.items():
        if tuple(sd[k].shape) != tuple(v.shape):
            raise ValueError("averaged weights: %s has shape %s, the model's is %s" % (k, tuple(sd[k].shape), tuple(v.shape)))
    dev = next(iter(ref.values())).device
    return torch.cat([sd[k].detach().reshape(-1).to(dev, torch.float32) for k in ref]).contiguous()


# ---------------------------------------------------------------- per-tensor statistics (qpn_tensor_stats) shared by FusedTrainer and FlatAdam
TENSOR_STAT_FIELDS = ("grad_norm", "weight_norm", "update_norm", "update_ratio", "grad_absmax", "weight_absmax", "grad_nonfinite")


def _tensor_lrs(n_tensors, positions, lrs):
    """learning rate of every tensor (model.parameters() order) from the groups' values and positions[g], the tensors group g holds; 0.0: in no group (frozen)"""
    out = [0.0] * n_tensors
    for ps, lr in zip(positions, lrs):
        for pos in ps:
            out[pos] = lr
    return out


def _tensor_stats(who, model, w, g, den_ptr, m, v, step, betas, eps, tensor_lrs):
    """One qpn_tensor_stats call over the flat buffers of `model` and its result as an ordered dict state_dict key -> {TENSOR_STAT_FIELDS}.  w, g, m, v: flat fp32
    CUDA tensors (g may hold a trailer behind the gradient; den_ptr: the address of its denominator, or None); `step`: the number of the latest Adam launch;
    tensor_lrs: the learning rate that launch used for every tensor.  update_norm = sqrt(update_sumsq) * (float32(lr) / bc1): the fp32 factor k_adam multiplies by."""
    dev = w.device
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("qpnet_amd.%s.tensor_stats: a synchronous diagnostic call (it drains the stream and reads records back) cannot be captured into a graph" % who)
    named = list(model.named_parameters())
    ends, o = [], 0
    for _, p in named:
        o += p.numel()
        ends.append(o)
    if o != w.numel():
        raise RuntimeError("qpnet_amd.%s.tensor_stats: the model's parameters hold %d elements, the flat vector %d" % (who, o, w.numel()))
    nt = len(ends)
    out = (_lib.QpnTensorStat * nt)()
    L, hd = model._native(dev)
    with torch.cuda.device(dev):
        _lib.check(L.qpn_tensor_stats(hd, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), o, step, betas[0], betas[1], eps, den_ptr,
                                      nt, (C.c_int64 * nt)(*ends), out, torch.cuda.current_stream(dev).cuda_stream))
    bc1 = np.float32(1.0 - float(np.float32(betas[0])) ** step)      # qpn_launch_adam's: fp64, rounded once
    res = collections.OrderedDict()
    for (key, _), r, lr in zip(named, out, tensor_lrs):
        wn = float(np.sqrt(r.weight_sumsq))
        un = float(np.sqrt(r.update_sumsq)) * float(np.float32(lr) / bc1)
        res[key] = {"grad_norm": float(np.sqrt(r.grad_sumsq)), "weight_norm": wn, "update_norm": un,
                    "update_ratio": un / wn if wn > 0.0 else (0.0 if un == 0.0 else float("inf")),
                    "grad_absmax": float(r.grad_absmax), "weight_absmax": float(r.weight_absmax), "grad_nonfinite": int(r.grad_nonfinite)}
    return res


# ---------------------------------------------------------------- Adam state in torch.optim.Adam's state_dict layout
_ADAM_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def adam_state_to_torch(model, m, v, steps, hyper, groups=None):
    """{"state": {i: {"step","exp_avg","exp_avg_sq"}}, "param_groups": [...]}: what torch.optim.Adam(model.parameters())
    .state_dict() holds after `steps` steps, built from the flat moment buffers (reference checkpoints store exactly this,
    src/bin/qpnet_train.py:346-352), so either side can resume the other's checkpoint.
    groups = [(hyper of the group, [positions of its tensors in model.parameters()])]: the layout of a torch.optim.Adam built with those groups -- one entry
    per group, "params" numbered consecutively across the groups in group order, "state" keyed by those numbers, tensors of no group (frozen) absent;
    `hyper` is not looked at then."""
    params = list(model.parameters())
    offs, o = [], 0
    for p in params:
        offs.append(o)
        o += p.numel()
    if groups is None:
        groups = [(hyper, list(range(len(params))))]
    state, out_groups, k = {}, [], 0
    for hyp, positions in groups:
        ids = []
        for pos in positions:
            p, o = params[pos], offs[pos]
            n = p.numel()
            if steps > 0 and m is not None:
                state[k] = {"step": torch.tensor(float(steps)), "exp_avg": m[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": v[o:o + n].view(p.shape).clone()}
            ids.append(k)
            k += 1
        group = dict(lr=hyp["lr"], betas=tuple(hyp["betas"]), eps=hyp["eps"], weight_decay=hyp["weight_decay"])
        group.update(_ADAM_GROUP_DEFAULTS)
        group["params"] = ids
        out_groups.append(group)
    return {"state": state, "param_groups": out_groups}


def adam_state_from_torch(model, sd, flat, groups=None):
    """inverse of adam_state_to_torch; also accepts the previous round's {"flat_adam": ...} format.  groups = [positions of the group's tensors]: the state of an
    optimizer with these groups -> (m, v, steps, [hyper of every group]); another number of groups, or a group of another size, raises ValueError (torch's rule)."""
    if groups is not None:
        sgs = sd["param_groups"]
        if len(sgs) != len(groups):
            raise ValueError("loaded state dict has a different number of parameter groups (%d, this optimizer has %d)" % (len(sgs), len(groups)))
        for gi, (sg, positions) in enumerate(zip(sgs, groups)):
            if len(sg["params"]) != len(positions):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group "
                                 "(group %d: %d parameters, this optimizer's has %d)" % (gi, len(sg["params"]), len(positions)))
            if sg.get("amsgrad"):
                raise ValueError("amsgrad Adam state cannot be resumed by the fused Adam kernel")
        params = list(model.parameters())
        offs, o = [], 0
        for p in params:
            offs.append(o)
            o += p.numel()
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        steps = 0
        for sg, positions in zip(sgs, groups):
            for key, pos in zip(sg["params"], positions):
                st = sd["state"].get(key)
                if st is not None:
                    o, n = offs[pos], params[pos].numel()
                    m[o:o + n] = st["exp_avg"].reshape(-1).to(flat.device, torch.float32)
                    v[o:o + n] = st["exp_avg_sq"].reshape(-1).to(flat.device, torch.float32)
                    steps = max(steps, int(float(st["step"])))
        return m, v, steps, [{k: sg[k] for k in ("lr", "betas", "eps", "weight_decay") if k in sg} for sg in sgs]
    if "flat_adam" in sd:
        st = sd["flat_adam"]
        return st["exp_avg"].to(flat.device).clone(), st["exp_avg_sq"].to(flat.device).clone(), int(st["step"]), dict(sd["param_groups"][0])
    params = list(model.parameters())
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    steps, o = 0, 0
    index = sd["param_groups"][0].get("params", list(range(len(params))))
    for pos, p in enumerate(params):
        n = p.numel()
        st = sd["state"].get(index[pos]) if pos < len(index) else None
        if st is not None:
            m[o:o + n] = st["exp_avg"].reshape(-1).to(flat.device, torch.float32)
            v[o:o + n] = st["exp_avg_sq"].reshape(-1).to(flat.device, torch.float32)
            steps = max(steps, int(float(st["step"])))
        o += n
    hyper = {k: sd["param_groups"][0][k] for k in ("lr", "betas", "eps", "weight_decay") if k in sd["param_groups"][0]}
    if sd["param_groups"][0].get("amsgrad"):
        raise ValueError("amsgrad Adam state cannot be resumed by the fused Adam kernel")
    return m, v, steps, hyper


# ---------------------------------------------------------------- parameter groups (qpn_adam_groups) shared by FusedTrainer and FlatAdam
class _AdamGroups:
    """The segment table of a grouped optimiser over one model's flat vector, as the C ABI takes it, and which tensors every group holds.
    seg_end / seg_group: the table; positions[g]: the positions in model.parameters() of group g's tensors, in the order state_dict() numbers them."""

    def __init__(self, n_groups, seg_end, seg_group, positions, numels):
        if n_groups > ADAM_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (got %d)" % (ADAM_MAX_GROUPS, n_groups))
        if not any(g >= 0 for g in seg_group):
            raise ValueError("parameter groups: every parameter is frozen (nothing to train)")
        self.n_groups, self.positions = n_groups, positions
        self.seg_end_list, self.seg_group_list = list(seg_end), list(seg_group)
        self.seg_end = (C.c_int64 * len(seg_end))(*seg_end)
        self.seg_group = (C.c_int32 * len(seg_group))(*seg_group)
        grouped = set(pos for ps in positions for pos in ps)
        self.n_trainable = sum(numels[pos] for pos in grouped)
        self.n_frozen = sum(numels) - self.n_trainable

    def send(self, model, L, hd, lrs, wds, stream):
        """make the handle's Adam launches use this table with these values (the same table again: no device work, only the values change).  The groups are
        sticky on the model's handle: the model remembers that they are on, so that an optimiser WITHOUT groups switches them off first (_groups_off)"""
        n = self.n_groups
        _lib.check(L.qpn_adam_groups(hd, n, (C.c_float * n)(*lrs), (C.c_float * n)(*wds), len(self.seg_end), self.seg_end, self.seg_group, stream))
        model.__dict__["_qpn_groups_on"] = True


def _groups_off(model, L, hd):
    """An optimiser without parameter groups is about to launch Adam on this model's handle: groups a grouped optimiser left there (a FusedTrainer / FlatAdam that
    froze tensors for the first N steps, say) are switched off -- its own lr / weight_decay apply to every element again.  A host-only call, made only when some
    optimiser has switched groups on since: a model that never had groups makes exactly the calls it always made."""
    if model.__dict__.get("_qpn_groups_on"):
        _lib.check(L.qpn_adam_groups(hd, 0, None, None, 0, None, None, None))
        model.__dict__["_qpn_groups_on"] = False


def _table_of_positions(group_of, numels):
    """group of every tensor (in model.parameters() order; -1: frozen) -> (seg_end, seg_group), a segment per run of one group"""
    seg_end, seg_group, o = [], [], 0
    for g, n in zip(group_of, numels):
        o += n
        if seg_group and seg_group[-1] == g:
            seg_end[-1] = o
        else:
            seg_end.append(o); seg_group.append(g)
    return seg_end, seg_group


def _check_group_value(name, v):
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError("parameter groups: %s must be a finite number >= 0, got %r" % (name, v))
    return v


def trainer_param_groups(model, param_groups):
    """FusedTrainer's `param_groups` -> (_AdamGroups, [lr_scale of every group], [weight_decay of every group]).  Entries are {"params": pattern or list of
    patterns over state_dict keys (fnmatch), "lr_scale": 1.0, "weight_decay": <the trainer's>, "frozen": False}.  Group 0 is the DEFAULT group: the parameters no
    entry matches, at the trainer's lr and weight_decay; every entry that is not frozen is a group of its own after it, in order.  Pure: works on a CPU model."""
    entries, scales, wds = [], [1.0], [None]
    for e in param_groups:
        if not isinstance(e, dict) or "params" not in e or set(e) - {"params", "lr_scale", "weight_decay", "frozen"}:
            raise ValueError('param_groups entries are dicts {"params": pattern(s), "lr_scale": 1.0, "weight_decay": ..., "frozen": False}, got %r' % (e,))
        if e.get("frozen", False):
            entries.append((e["params"], ADAM_FROZEN))
            continue
        entries.append((e["params"], len(scales)))
        scales.append(_check_group_value("lr_scale", e.get("lr_scale", 1.0)))
        wds.append(None if e.get("weight_decay") is None else _check_group_value("weight_decay", e["weight_decay"]))
    if len(scales) > ADAM_MAX_GROUPS:
        raise ValueError("at most %d parameter groups, the default group included (got %d)" % (ADAM_MAX_GROUPS, len(scales)))
    seg_end, seg_group, key_group = adam_group_table(model.cfg, entries, 0)
    keys = list(key_group)                              # (layout order = state_dict order = model.parameters() order)
    named = [k for k, _ in model.named_parameters()]
    if named != keys:
        raise ValueError("parameter groups: the model's parameters are not the layout of its configuration")
    numels = [p.numel() for p in model.parameters()]
    positions = [[i for i, k in enumerate(keys) if key_group[k] == g] for g in range(len(scales))]
    return _AdamGroups(len(scales), seg_end, seg_group, positions, numels), scales, wds


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (lr, betas, eps, weight_decay; no amsgrad) as ONE kernel over the model's flat parameter
    buffer -- a one-line swap for `torch.optim.Adam(model.parameters(), lr=...)` in the reference loop
    (src/bin/qpnet_train.py:426-429,531), whose 120-tensor foreach update costs 0.9 ms per step on this GPU.
    Gradients are read from `p.grad`: when they are consecutive views of one flat buffer (what the autograd backward hands
    out) no gather happens.  state_dict()/load_state_dict() use torch.optim.Adam's own layout, so checkpoints written by
    the reference trainer resume here and vice versa.
    max_grad_norm=c: `torch.nn.utils.clip_grad_norm_(model.parameters(), c)` in front of every step, inside the step's launches (qpn_adam_step_clip); p.grad is
    left unscaled.  A step whose gradient norm is not finite applies nothing and raises QpnError(-4) at the next status collection.
    ema_decay=d (0 < d < 1): `.ema`, a flat fp32 average of the weights seeded with them, moves inside the same launch with every APPLIED update
    (qpn_adam_step_avg: e += (w_new - e) * (1 - d)); ema_state_dict() / load_ema() as FusedTrainer's.
    params=[{"params": [tensors of this model], "lr": ..., "weight_decay": ...}, ...]: torch-style parameter groups (at most 8), each with a learning rate and a
    weight decay of its own inside the same launch (qpn_adam_groups); parameters of the model in no group are frozen, as if they had not been passed to
    torch.optim.Adam.  betas / eps must agree across the groups.  `param_groups` are torch's own (lr schedulers act per group: the values are sent with every
    step), and state_dict() / load_state_dict() have the layout of a torch.optim.Adam built with the same groups."""

    def __init__(self, model, params=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, ema_decay=None):
        self.model = model
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)      # (a setting of this object, not of the checkpoint: state_dict() keeps torch.optim.Adam's layout)
        self.ema_decay = _check_ema_decay(ema_decay)
        self.ema = None
        super().__init__(list(model.parameters()) if params is None else params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._groups = None if params is None else self._make_groups()
        self._grouped = params is not None
        self._m = self._v = None
        self._steps = 0
        self._applied_base = None     # clipping on: (steps, the handle's applied-update count) at the first step (a skipped non-finite step must not advance the bias correction)

    def _make_groups(self):
        mparams = list(self.model.parameters())
        pos_of = {id(p): i for i, p in enumerate(mparams)}
        group_of, positions = [ADAM_FROZEN] * len(mparams), []
        for gi, g in enumerate(self.param_groups):
            ps = []
            for p in g["params"]:
                if id(p) not in pos_of:
                    raise ValueError("FlatAdam: group %d holds a tensor that is not a parameter of this model" % gi)
                group_of[pos_of[id(p)]] = gi
                ps.append(pos_of[id(p)])
            positions.append(ps)
        self._groups_agree()
        numels = [p.numel() for p in mparams]
        seg_end, seg_group = _table_of_positions(group_of, numels)
        return _AdamGroups(len(self.param_groups), seg_end, seg_group, positions, numels)

    def add_param_group(self, param_group):
        """torch's own (it also builds the groups inside __init__); on a grouped optimiser a group added later rebuilds the segment table, with every check of the
        constructor (a tensor of this model, at most 8 groups, betas / eps in agreement).  The moments are flat over the whole model: a tensor that was frozen so
        far starts from zero moments, at the optimiser's step count."""
        super().add_param_group(param_group)
        if self.__dict__.get("_grouped"):
            try:
                self._groups = self._make_groups()
            except ValueError:
                self.param_groups.pop()                 # (refused: the optimiser is what it was)
                raise

    def _groups_agree(self):
        g0 = self.param_groups[0]
        for gi, g in enumerate(self.param_groups):
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise ValueError("FlatAdam: betas / eps must agree across the parameter groups (group %d has betas=%r eps=%r, group 0 betas=%r eps=%r)"
                                 % (gi, g["betas"], g["eps"], g0["betas"], g0["eps"]))

    def _applied(self, L, hd, dev):
        n = C.c_int64(0)
        with torch.cuda.device(dev):
            _lib.check(L.qpn_train_applied_updates(hd, C.byref(n), torch.cuda.current_stream(dev).cuda_stream))
        return int(n.value)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        model = self.model
        flat = getattr(model, "_flat", None)
        if flat is None:
            raise RuntimeError("FlatAdam.step before the first forward/backward of the model")
        dev = flat.device
        L, hd = model._native(dev)
        clipping = self.max_grad_norm > 0.0
        if clipping:
            # a step whose gradient norm was not finite applies nothing and is reported by whichever call collects the status word next (the next forward, backward,
            # check_status()): when a status error has been raised anywhere since this optimizer's last step, the step count -- the bias correction's exponent, and what
            # state_dict() stores -- is set back to the updates the device applied (one stream drain, on that path only)
            if self._applied_base is None:
                self._applied_base = (self._steps, self._applied(L, hd, dev), _lib.STATUS_ERRORS[0])      # (once per optimizer: drains the stream)
            elif _lib.STATUS_ERRORS[0] != self._applied_base[2]:
                applied = self._applied(L, hd, dev)
                self._steps = self._applied_base[0] + applied - self._applied_base[1]
                self._applied_base = (self._steps, applied, _lib.STATUS_ERRORS[0])
        with torch.cuda.device(dev):
            _lib.check(L.qpn_train_status_collect(hd))       # a pending forward check (no-op after a backward has collected it)
        params = model_params(model)
        g = _flat_grad_of(params)
        if g is None:                                # grads came from elsewhere (or some are None): gather them
            g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
        if self._m is None or self._m.numel() != flat.numel() or self._m.device != dev:
            m0, v0 = self._m, self._v
            self._m = torch.zeros_like(flat); self._v = torch.zeros_like(flat)
            if m0 is not None and m0.numel() == flat.numel():
                self._m.copy_(m0); self._v.copy_(v0)
        grp = self.param_groups[0]
        self._steps += 1
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            if self._groups is not None:             # (every step: a scheduler may have moved a group's lr; the same table again costs no device work)
                self._groups_agree()
                self._groups.send(model, L, hd, [pg["lr"] for pg in self.param_groups], [pg["weight_decay"] for pg in self.param_groups], stream)
            else:
                _groups_off(model, L, hd)
            averaging = self.ema_decay > 0.0
            if averaging:
                self.ema = _ema_home(self.ema, flat)
            _lib.check(L.qpn_adam_step_avg(hd, flat.data_ptr(), g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), flat.numel(),
                                           self._steps, grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], None,
                                           self.max_grad_norm, self.ema.data_ptr() if averaging else None, self.ema_decay if averaging else 0.0, stream))
            if clipping:
                _lib.check(L.qpn_train_status_enqueue(hd, stream))      # (a non-finite norm is this launch's own finding: the next collection reports it)
        return loss

    def _hyper(self):
        return {k: self.param_groups[0][k] for k in ("lr", "betas", "eps", "weight_decay")}

    def tensor_stats(self, weights="model"):
        """FusedTrainer.tensor_stats for this optimizer's latest step(): the gradient is the parameters' `.grad` as they are now (the step left them alone),
        the learning rates are the groups' current ones.  RuntimeError before the first step and on a capturing stream."""
        if weights not in ("model", "ema"):
            raise ValueError('tensor_stats: weights must be "model" or "ema", got %r' % (weights,))
        if weights == "ema" and self.ema_decay <= 0.0:
            raise RuntimeError('tensor_stats(weights="ema"): this optimizer keeps no averaged weights (ema_decay is off)')
        model = self.model
        flat = getattr(model, "_flat", None)
        if self._steps < 1 or self._m is None or flat is None or not flat.is_cuda or self._m.device != flat.device:
            raise RuntimeError("qpnet_amd.FlatAdam.tensor_stats before the first update: there is no Adam launch to describe")
        params = model_params(model)
        g = _flat_grad_of(params)
        if g is None:
            g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
        grp = self.param_groups[0]
        if self._groups is not None:
            lrs = _tensor_lrs(len(params), self._groups.positions, [pg["lr"] for pg in self.param_groups])
        else:
            lrs = [grp["lr"]] * len(params)
        w = _ema_home(self.ema, flat) if weights == "ema" else flat
        return _tensor_stats("FlatAdam", model, w, g, None, self._m, self._v, self._steps, grp["betas"], grp["eps"], lrs)

    def ema_state_dict(self):
        """the averaged weights under the model's state_dict() keys ({} with averaging off); not part of state_dict(), which keeps torch.optim.Adam's layout."""
        return _ema_to_state_dict(self.model, self.ema) if self.ema_decay > 0.0 else {}

    def load_ema(self, sd):
        """restore the average from an ema_state_dict(); None: seed it from the current weights at the next step."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("load_ema: this optimizer keeps no averaged weights (ema_decay is off)")
        self.ema = None if sd is None else _ema_from_state_dict(self.model, sd)

    def state_dict(self):
        if self._groups is not None:
            groups = [({k: pg[k] for k in ("lr", "betas", "eps", "weight_decay")}, ps) for pg, ps in zip(self.param_groups, self._groups.positions)]
            return adam_state_to_torch(self.model, self._m, self._v, self._steps, None, groups)
        return adam_state_to_torch(self.model, self._m, self._v, self._steps, self._hyper())

    def load_state_dict(self, sd):
        params = list(self.model.parameters())
        flat = getattr(self.model, "_flat", None)
        if flat is None:
            flat = torch.cat([p.detach().reshape(-1).float() for p in params])
        if self._groups is not None:
            self._m, self._v, self._steps, hypers = adam_state_from_torch(self.model, sd, flat, self._groups.positions)
            for pg, hyper in zip(self.param_groups, hypers):
                pg.update(hyper)
            return
        self._m, self._v, self._steps, hyper = adam_state_from_torch(self.model, sd, flat)
        for k, v in hyper.items():
            if k != "params":
                self.param_groups[0][k] = v


class FusedTrainer:
    """forward + mean CE + backward + Adam entirely behind the C ABI (flat fp32 buffers).

    Mirrors the loop body of the reference trainer (src/bin/qpnet_train.py:517-531) with
    torch.optim.Adam(lr=1e-4, betas=(0.9,0.999), eps=1e-8, weight_decay=0) semantics.
    With world_size > 1 every rank's gradient is weighted by its row count inside the gradient-reduction kernel, summed
    over ranks with ONE RCCL all-reduce of the flat buffer (the row counts ride in its last element) and divided by the
    global row count inside the Adam kernel: the update is the gradient of the mean CE over ALL ranks' rows, with no
    extra elementwise launch or allocation in the step.
    state_dict()/load_state_dict() use torch.optim.Adam's layout (resume of reference-made checkpoints and vice versa).
    max_grad_norm=c (None / 0: off): the step clips like `torch.nn.utils.clip_grad_norm_(model.parameters(), c)` between backward and Adam.step -- data-parallel: the
    norm of the exchanged, averaged gradient -- inside the library's optimiser step; `last_grad_norm` is the norm (before clipping) that belongs to the loss
    step() / flush_loss() last returned (None when that was None, or clipping is off).  A non-finite norm skips the update and raises like the other status errors.
    A trainer setting: it is not part of state_dict().
    ema_decay=d (None / 0: off; 0 < d < 1): `ema`, a flat fp32 exponential moving average of the weights, seeded with a copy of them at the first step, moves inside
    the Adam launch itself with every APPLIED update: e += (w_new - e) * (1 - d) -- a step the device skipped (a flagged chunk, a peer's flag, a non-finite norm)
    leaves it alone.  No launch, copy or wait is added to a step.  ema_state_dict() / load_ema() carry it through checkpoints (loaders.save_checkpoint writes it as
    "ema" next to "model"), forward_loss(weights="ema") scores it on held-out data; it is not part of state_dict() either.
    accum_steps=K (a plain int >= 1; 1: off): gradient accumulation -- step() becomes a MICRO-step, and one Adam update is applied per window of K of them, to the
    gradient of the mean CE over all the window's rows (chunks of unequal batch_length get their row weights: the window is the sum a data-parallel step takes over
    ranks, taken over time, so one GPU follows the trajectory of a K-rank run).  `micro_step` is the position in the open window (0 .. K-1); step_count, the bias
    correction and state_dict()'s step numbers count UPDATES.  Single rank: still one foreign call per micro-step (qpn_train_step_acc); a micro-step that does not
    close its window returns its own loss, and last_grad_norm is None with it (no norm launch ran).  world_size > 1: every micro-step runs call by call, only the closing
    one exchanges -- the accumulator, ONCE per window -- and runs Adam; the two-bucket split is not used (it is taken as agreed to be off: K is the same on every rank,
    so every rank issues the same single collective per window).  Clipping and the average apply to the update, i.e. once per window.  A flagged micro-step leaves its
    flag in the accumulator's trailer and the closing Adam launch skips.  After a device-side status error (QpnError -4 / -2 from any call) the open window is ABANDONED:
    the next step() is micro-step 0 and overwrites the accumulator, the chunks accumulated so far are dropped as the flagged chunk itself is.  Under stream capture
    with K > 1 step() raises (one captured graph cannot hold both kinds of micro-step).  A trainer setting like max_grad_norm: not part of state_dict(), no accumulator
    reaches a checkpoint.  K = 1 makes exactly the calls made without the option.
    param_groups=[{"params": pattern or list of patterns, "lr_scale": 1.0, "weight_decay": <the trainer's>, "frozen": False}, ...] (None: off): parameter groups by
    fnmatch patterns over state_dict keys, inside the same Adam launch (qpn_adam_groups).  A frozen entry's tensors are not updated (weights and moments stay bit for
    bit; their gradient is left out of the clipping norm); every other entry trains at lr * lr_scale (an fp32 product, formed from the current `lr` at every step)
    with its own weight decay; parameters no entry matches form the default group at the trainer's lr and weight_decay.  At most 8 groups, the default one included.
    Works on every host path (the one-call step, accum_steps > 1, world_size > 1 -- the groups must be the same on every rank, as the other hyper-parameters must).
    A trainer setting like max_grad_norm; with it state_dict() / load_state_dict() have the layout of a torch.optim.Adam built with the same groups (default
    group first when it is not empty, frozen tensors absent).  load_state_dict() with groups takes from the file: the moments and the step count; betas and eps; the
    base `lr` (the file's lr of the first group whose lr_scale is not 0, divided by that scale); the trainer's `weight_decay` when the file has the default group.
    lr_scale and the entries' own weight decays stay this trainer's.  `n_trainable` / `n_frozen` count the elements.  The groups are sticky on the model's native
    handle: an optimiser without groups (a FusedTrainer / FlatAdam built later on the same model, a stock Adam stepped by the hooks) switches them off before its launch.
    distill={"teacher": QPNet, "alpha": a, "temperature": T} (None: off): knowledge distillation -- every step's loss is the soft-target loss
    (1 - a) CE(z, y) + a T^2 KL(softmax(t / T) || softmax(z / T)), mean over the rows (qpn_train_distill), t the teacher's logits for the same chunk:
    step() runs the teacher's teacher-forced forward on the current stream (its own native handle and flat weights, the same inputs) into a buffer it keeps, arms the
    student's handle and runs the step it would have run, on every host path (the one-call step, every micro-step of accum_steps > 1, world_size > 1).  The armed step
    leaves the fused post-net tile (the forward writes the logits, one kernel computes the loss and dL/dlogits, the backward computes the post-net itself:
    profiles/distill.txt has the cost).  The teacher must share n_quantize, n_aux and upsampling_factor with the student (ValueError otherwise, as for 0 < a <= 1 and a
    finite T > 0, both as float32 numbers); its stack may differ -- feed chunks cut for the larger receptive field (runners.joint_fields).  The teacher is never written
    and gets no optimiser; its own status word is collected where the student's is and raises naming the teacher.  step(teacher_logits=...) takes precomputed logits
    instead (a cached teacher, an ensemble average), the "teacher" entry may then be absent.  A NaN or an infinity among the teacher logits skips the update and raises
    QpnError(-4) ("... teacher logits ...") like the other status errors.  step() / flush_loss() return the distillation total; forward_loss() and score() stay the
    plain cross entropy.  A step being captured raises.  A trainer setting: not part of state_dict(), the teacher reaches no checkpoint.
    ignore_index=k / label_smoothing=eps / loss_norm="rows" | "weights" and step(sample_weights=w): the criterion's options ("Loss options";
    qpn_train_loss_opts) -- what torch.nn.CrossEntropyLoss(ignore_index=, label_smoothing=) or reduction="none" times a mask gives.  Per row, w_r = w[b, t] (1 without
    weights), 0 where the target equals ignore_index; the loss is (1 / N) sum_r w_r (lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q) with N the chunk's row count
    ("rows", the default: the row-weighted combination over ranks and accumulation windows stays exact) or sum_r w_r ("weights": torch's `mean` with ignore_index;
    only with accum_steps=1 and world_size=1 -- ValueError otherwise, as for eps outside [0, 1) or label_smoothing together with distill=).  Rows of weight 0 are not
    read and their targets are not range-checked.  With distill= the weights multiply the whole row loss.  A NaN, infinite or negative weight skips the update and
    raises QpnError(-4) ("... sample weights ...").  A step with any option set leaves the fused post-net tile as a distillation step does (profiles/loss_options.txt has
    the cost); with every option at its default the step makes exactly the calls it always made.  forward_loss() and score() stay the plain cross entropy.  A step
    being captured raises.  Trainer settings: not part of state_dict()."""

    # The device-side status word (bad taps / targets; the reference asserts in-line, qpnet.py:294, qpnet_train.py:525) is copied to pinned
    # memory behind every step; a step starts by looking at the copy made TWO steps earlier (the previous step is still queued on the
    # device while the host enqueues this one: waiting for it would idle the GPU).  A bad chunk is raised two steps late at most, not up to 99
    # as when the word was read every 100 steps.  check_status() collects everything outstanding.

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, process_group=None, world_size=1, max_grad_norm=None, ema_decay=None,
                 accum_steps=1, param_groups=None, distill=None, ignore_index=None, label_smoothing=0.0, loss_norm="rows"):
        self.model = model
        self._distill = _check_distill(model, distill)      # None, or (teacher or None, alpha, temperature)
        self._loss_ignore, self._loss_eps, self._loss_norm = _check_loss_options(ignore_index, label_smoothing, loss_norm)
        if self._loss_eps > 0.0 and self._distill is not None:
            raise ValueError("label_smoothing cannot be combined with distill= (the soft targets already smooth)")
        if self._loss_norm == 1 and (_check_accum_steps(accum_steps) > 1 or world_size > 1):
            raise ValueError('loss_norm="weights" divides by one chunk\'s sum of weights: it needs accum_steps=1 and world_size=1 (got %r and %r); "rows" combines '
                             "exactly over ranks and accumulation windows" % (accum_steps, world_size))
        self._teacher_logits = None                         # the teacher's (B, BL, Q) output, kept from step to step
        self._groups = self._group_scales = self._group_wds = None
        if param_groups is not None:
            self._groups, self._group_scales, self._group_wds = trainer_param_groups(model, param_groups)
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self.ema_decay = _check_ema_decay(ema_decay)
        self.accum_steps = _check_accum_steps(accum_steps)
        self._micro = 0               # position in the open accumulation window
        self.acc = None               # accum_steps > 1: the window's summed row-weighted gradient + trailer
        self.ema = None               # averaging on: the flat average, from the first step (or load_ema) on
        self.last_grad_norm = None
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.step_count = 0
        self.m = self.v = self.g = None
        self.pg, self.world = process_group, world_size
        self._logits = None
        self.last_buckets = (0, 0)
        self._applied_base = None     # (step_count, the handle's applied-update count) at this trainer's first step / after a re-base (see _rebase_step_count)
        self._early = None            # the stream the early bucket of the gradient exchange runs on (world_size > 1)
        self._two_buckets = None      # agreed over the process group at the first data-parallel step (every rank must issue the same collectives)
        if self.accum_steps > 1:
            self._two_buckets = False  # (accumulating: one exchange of the accumulator per window, on every rank)

    @property
    def n_trainable(self):
        """elements of the flat parameter vector this trainer updates"""
        return self._groups.n_trainable if self._groups is not None else sum(p.numel() for p in self.model.parameters())

    @property
    def n_frozen(self):
        return self._groups.n_frozen if self._groups is not None else 0

    def _group_values(self):
        """(lr, weight_decay) of every group now: lr_g = float32(lr) * float32(lr_scale_g)"""
        lr = np.float32(self.lr)
        return ([float(lr * np.float32(sc)) for sc in self._group_scales],
                [float(self.wd if wd is None else wd) for wd in self._group_wds])

    @property
    def micro_step(self):
        """position of the next step() in the open accumulation window: 0 .. accum_steps - 1 (always 0 with accum_steps = 1)"""
        return self._micro

    def _buffers(self, flat):
        if self.m is None or self.m.device != flat.device or self.m.numel() != flat.numel():
            m0, v0 = self.m, self.v
            self.m = torch.zeros_like(flat); self.v = torch.zeros_like(flat)
            if m0 is not None and m0.numel() == flat.numel():
                self.m.copy_(m0); self.v.copy_(v0)
        if self.g is None or self.g.device != flat.device or self.g.numel() != flat.numel() + 4:
            self.g = torch.empty(flat.numel() + 4, dtype=torch.float32, device=flat.device)   # gradient + trailer (row count)
        if self.ema_decay > 0.0:
            self.ema = _ema_home(self.ema, flat)
        if self.accum_steps > 1 and (self.acc is None or self.acc.device != flat.device or self.acc.numel() != flat.numel() + 4):
            self.acc = torch.empty(flat.numel() + 4, dtype=torch.float32, device=flat.device)     # (micro-step 0 overwrites it: never cleared)
            self._micro = 0

    @staticmethod
    def _norm(t, dtype, dev):
        return t if (t.dtype == dtype and t.device == dev and t.is_contiguous()) else t.to(dev, dtype).contiguous()

    def step(self, x, h, t, d, blength, want_loss=True, maxd=None, h_grad=None, teacher_logits=None, sample_weights=None):
        """One optimisation step.  maxd = ceil(max(d)) of the chunk; a loader that built d on the host (the reference's
        train_generator does, qpnet_train.py:268-272) passes it in, otherwise it is read back from the device (one sync).
        Inputs are normalised like QPNet.forward does (int64 samples/targets, float32 features/factors, contiguous).
        h_grad: an optional float32 CUDA tensor shaped like `h`, contiguous, on the inputs' device (anything else: ValueError before any device work).  The step's
        backward fills it, stream-ordered, with d(mean CE of THIS chunk) / dh at the weights the forward saw (the Adam launch comes behind it), every element, exact
        zeros in the frames no row of the chunk reaches.  With accum_steps > 1 every micro-step takes its own; with world_size > 1 it is the local chunk's gradient,
        nothing is exchanged; the row-count weighting of either never enters it.  A step that is being captured raises with it; after a step whose status word
        is set its contents are unspecified.
        teacher_logits: with distill= set, precomputed teacher logits for this chunk -- float32, CUDA, contiguous, (B, BL, n_quantize), on the inputs' device
        (anything else: ValueError before any device work) -- in the place of a forward of distill["teacher"] (which may then be absent).
        sample_weights: per-row weights of this chunk's loss -- float32, CUDA, contiguous, (B, BL), on the inputs' device (anything else: ValueError before any
        device work); see the class docstring (ignore_index / label_smoothing / loss_norm)."""
        if sample_weights is None and self._loss_ignore is None and self._loss_eps == 0.0 and self._loss_norm == 0:
            return self._step_plain(x, h, t, d, blength, want_loss, maxd, h_grad, teacher_logits)
        # loss options: arm the handle, then the step as ever -- its forward-with-loss consumes the arm and runs k_ce_hard<NV, true> (with distill=:
        # k_ce_soft<NV, true>) where the cross entropy ran.  Every micro-step of an accumulation window, and every host path, is armed this way.
        dev = x.device
        if sample_weights is not None:
            _check_step_tensor("sample_weights", "(B, BL)", sample_weights, (x.shape[0], int(blength[0])), dev)
        if dev.type != "cuda":
            raise RuntimeError("qpnet_amd.FusedTrainer runs on an AMD GPU only (tensors are on %s)" % dev)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("qpnet_amd.FusedTrainer: a step cannot be captured into a graph with loss options (sample_weights / ignore_index / label_smoothing / "
                               "loss_norm: the arm is host state a replay would not renew)")
        L, hd = self.model._native(dev)
        opts = _make_loss_opts(sample_weights, self._loss_ignore, self._loss_eps, self._loss_norm)
        try:
            _lib.check(L.qpn_train_loss_opts(hd, C.byref(opts)))
            return self._step_plain(x, h, t, d, blength, want_loss, maxd, h_grad, teacher_logits)
        finally:
            L.qpn_train_loss_opts(hd, None)              # (consumed by the step's forward; a step that raised in front of it must not leave the arm behind)

    def _step_plain(self, x, h, t, d, blength, want_loss, maxd, h_grad, teacher_logits):
        if self._distill is not None or teacher_logits is not None:
            return self._distill_step(x, h, t, d, blength, want_loss, maxd, h_grad, teacher_logits)
        if h_grad is None:
            return self._step(x, h, t, d, blength, want_loss, maxd)
        _check_h_grad(h_grad, h, x.device)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("qpnet_amd.FusedTrainer.step(h_grad=...): a step cannot be captured into a graph with a feature gradient (the request is host "
                               "state a replay would not renew)")
        dev = x.device
        L, hd = self.model._native(dev)
        _arm_input_grad(L, hd, h_grad)
        try:
            return self._step(x, h, t, d, blength, want_loss, maxd)
        finally:
            L.qpn_train_input_grad(hd, None, 0)          # (consumed by the step's backward; a step that raised in front of it must not leave the request behind)

    def _distill_step(self, x, h, t, d, blength, want_loss, maxd, h_grad, teacher_logits):
        """step() with the soft-target loss: the teacher's teacher-forced forward (or the logits handed in) on the current stream, the arm, then the step as ever --
        its forward-with-loss consumes the arm and runs k_ce_soft where the cross entropy ran.  Every micro-step of an accumulation window is armed this way."""
        model = self.model
        if self._distill is None:
            raise ValueError('step(teacher_logits=...) needs the trainer\'s distill={"alpha": a, "temperature": T}')
        teacher, alpha, temp = self._distill
        dev = x.device
        BL = int(blength[0])
        if teacher_logits is not None:
            _check_step_tensor("teacher_logits", "(B, BL, n_quantize)", teacher_logits, (x.shape[0], BL, model.n_quantize), dev)
        elif teacher is None:
            raise ValueError('distill without a "teacher" needs step(teacher_logits=...) at every step')
        if h_grad is not None:
            _check_h_grad(h_grad, h, dev)
        if dev.type != "cuda":
            raise RuntimeError("qpnet_amd.FusedTrainer runs on an AMD GPU only (tensors are on %s)" % dev)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("qpnet_amd.FusedTrainer(distill=...): a step cannot be captured into a graph with the soft-target loss (the arm is host state a "
                               "replay would not renew)")
        L, hd = model._native(dev)
        Lt = ht = None
        if teacher_logits is None:
            join_staged(x, dev, h, t, d)
            x = self._norm(x, torch.int64, dev); h = self._norm(h, torch.float32, dev); d = self._norm(d, torch.float32, dev)
            if maxd is None:
                maxd = int(torch.max(d.ceil()))
            B, T = x.shape
            if self._teacher_logits is None or self._teacher_logits.shape != (B, BL, model.n_quantize) or self._teacher_logits.device != dev:
                self._teacher_logits = torch.empty((B, BL, model.n_quantize), dtype=torch.float32, device=dev)
            teacher_logits = self._teacher_logits
            Lt, ht = teacher._native(dev)
            tflat = ensure_flat(teacher, dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            with torch.cuda.device(dev):
                # the teacher's own status word (a tap of ITS stack outside the layer input): collected where the student's is, at the same lag
                self._teacher_check(Lt, Lt.qpn_train_status_collect_lagged(ht))
                self._teacher_check(Lt, Lt.qpn_train_forward(ht, tflat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd,
                                                             x.data_ptr(), h.data_ptr(), d.data_ptr(), teacher_logits.data_ptr(), stream))
                self._teacher_check(Lt, Lt.qpn_train_status_enqueue(ht, stream))
        try:
            _lib.check(L.qpn_train_distill(hd, teacher_logits.data_ptr(), teacher_logits.numel(), alpha, temp))
            _arm_input_grad(L, hd, h_grad)
            out = self._step(x, h, t, d, blength, want_loss, maxd)
        finally:
            L.qpn_train_distill(hd, None, 0, 0.0, 1.0)       # (consumed by the step's forward; a step that raised in front of it must not leave the arm behind)
            if h_grad is not None:
                L.qpn_train_input_grad(hd, None, 0)
        if ht is not None and want_loss and want_loss != "lagged":
            with torch.cuda.device(dev):                     # (the stream has just been drained for the loss: in-step, like the student's own check)
                self._teacher_check(Lt, Lt.qpn_train_status_collect(ht))
        return out

    @staticmethod
    def _teacher_check(Lt, rc):
        if rc != 0:
            if rc in (-4, -2):
                _lib.STATUS_ERRORS[0] += 1
            raise _lib.QpnError(rc, "the distillation teacher's forward: " + Lt.qpn_last_error().decode("utf-8", "replace"))

    def _step(self, x, h, t, d, blength, want_loss, maxd):
        model = self.model
        dev = x.device
        if dev.type != "cuda":
            raise RuntimeError("qpnet_amd.FusedTrainer runs on an AMD GPU only (tensors are on %s)" % dev)
        L, hd = model._native(dev)
        flat = ensure_flat(model, dev)
        self._buffers(flat)
        join_staged(x, dev, h, t, d)
        x = self._norm(x, torch.int64, dev); t = self._norm(t, torch.int64, dev)
        h = self._norm(h, torch.float32, dev); d = self._norm(d, torch.float32, dev)
        assert x.dim() == 2 and t.shape[0] == x.shape[0] and h.dim() == 3 and h.shape[1] == model.n_aux and d.dim() == 2
        BL = int(blength[0])
        if maxd is None:
            maxd = int(torch.max(d.ceil()))
        B, T = x.shape
        if self._logits is None or self._logits.shape != (B, BL, model.n_quantize) or self._logits.device != dev:
            self._logits = torch.empty((B, BL, model.n_quantize), dtype=torch.float32, device=dev)
            self._dlogits = torch.empty_like(self._logits)
        stream = torch.cuda.current_stream(dev).cuda_stream
        loss = C.c_double(0.0)
        multi = self.world > 1
        if self._groups is not None:                   # (every step: lr may have moved; the same table again costs no device work)
            lrs, wds = self._group_values()
            with torch.cuda.device(dev):
                self._groups.send(model, L, hd, lrs, wds, stream)
        else:
            with torch.cuda.device(dev):
                _groups_off(model, L, hd)
        if self._applied_base is None and not torch.cuda.is_current_stream_capturing():
            n = C.c_int64(0)
            with torch.cuda.device(dev):
                _lib.check(L.qpn_train_applied_updates(hd, C.byref(n), stream))      # (once per trainer: drains the stream before its first step)
            self._applied_base = (self.step_count, int(n.value))
        # (a step being captured into a hipGraph -- torch.cuda.graph -- may not wait for events or read anything back: no status bookkeeping, the
        #  caller checks with check_status() outside the graph; the library runs the stack as a launch per layer while a stream is capturing)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self.accum_steps > 1:
            raise RuntimeError("qpnet_amd.FusedTrainer(accum_steps=%d): a step cannot be captured into a graph while accumulating (the micro-steps of a window "
                               "do not make the same launches)" % self.accum_steps)
        if not multi and not capturing:
            return self._step_call(L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, loss)
        self.last_grad_norm = None
        try:
            return self._step_calls(L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, multi, capturing, loss)
        except _lib.QpnError as e:
            if e.code in (-4, -2):                     # (QPN_ERANGE / QPN_ENODEV: what the device-side status word raises)
                self._micro = 0                        # (the open accumulation window is abandoned)
                self._rebase_step_count(L, hd, dev, stream, 0)
            raise

    def _step_call(self, L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, loss):
        """One rank, not capturing: the whole step -- or, with accum_steps > 1, the micro-step -- behind ONE foreign call (qpn_train_step_acc: the calls of
        _step_calls in their order; averaging, clipping and the window are its arguments, None / 0 where off).  While it runs the interpreter is free for the
        loader thread: the runner loop was bound by the two threads' interleaved Python, not by the device.  The update number it passes is the same for every
        micro-step of a window; step_count moves when the window closes."""
        K, micro = self.accum_steps, self._micro
        closing = micro == K - 1
        valid, norm = C.c_int(0), C.c_double(0.0)
        mode = 1 if want_loss == "lagged" else (2 if want_loss else 0)
        clip = self.max_grad_norm
        with torch.cuda.device(dev):
            rc = L.qpn_train_step_acc(hd, flat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd, x.data_ptr(), h.data_ptr(), d.data_ptr(),
                                      t.data_ptr(), t.shape[1], self._logits.data_ptr(), self._dlogits.data_ptr(), self.g.data_ptr(),
                                      self.m.data_ptr(), self.v.data_ptr(), flat.numel(), self.step_count + 1, self.lr, self.betas[0], self.betas[1],
                                      self.eps, self.wd, mode, C.byref(loss), C.byref(valid), clip, C.byref(norm),
                                      self.ema.data_ptr() if self.ema is not None else None, self.ema_decay if self.ema is not None else 0.0,
                                      self.acc.data_ptr() if K > 1 else None, micro, K, stream)
        if K > 1 and rc in (-4, -2):
            self._micro = 0                            # a device-side status error: the open window is abandoned, the next step() overwrites the accumulator
        elif closing:
            self._micro = 0
            self.step_count += 1
        else:
            self._micro = micro + 1
        if clip <= 0.0:
            pass                                       # (no clipping: there is no norm, last_grad_norm is left alone)
        elif not valid.value:
            self.last_grad_norm = None
        elif mode == 1:
            self.last_grad_norm = self._collected_norm(L, hd)      # (None where the step that loss belongs to ran unclipped or did not close a window: the C call hands back 0.0 there)
        else:
            self.last_grad_norm = norm.value if closing else None
        if rc:
            self._rebase_step_count(L, hd, dev, stream, rc)
        return loss.value if valid.value else None

    def _rebase_step_count(self, L, hd, dev, stream, rc):
        """A device-side status error: the Adam kernel skipped the flagged step's update and that of every step enqueued behind it until the host collected the
        word (k_adam), so the host's step count -- the bias correction's exponent, and what checkpoints store -- has run ahead of the updates applied.  It is set back
        to (count at the base) + (updates the device applied since): one stream drain, on the error path only.  rc != 0: raise it afterwards."""
        msg = L.qpn_last_error()                       # (the call below would replace it)
        if self._applied_base is not None:
            n = C.c_int64(0)
            with torch.cuda.device(dev):
                if L.qpn_train_applied_updates(hd, C.byref(n), stream) == 0:
                    self.step_count = self._applied_base[0] + int(n.value) - self._applied_base[1]
        if rc:
            raise _lib.QpnError(rc, msg.decode("utf-8", "replace"))

    def _step_calls(self, L, hd, dev, flat, stream, x, h, t, d, B, T, BL, maxd, want_loss, multi, capturing, loss):
        with torch.cuda.device(dev):
            if not capturing:
                _lib.check(L.qpn_train_status_collect_lagged(hd))   # the check of the step before the previous one (never waits for queued work)
            # forward + CrossEntropyLoss + dL/dlogits in one call (the loss stays on the device unless asked for)
            _lib.check(L.qpn_train_forward_loss(hd, flat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd,
                                                x.data_ptr(), h.data_ptr(), d.data_ptr(), t.data_ptr(), t.shape[1],
                                                self._logits.data_ptr(), 2, self._dlogits.data_ptr(), stream))      # (2: the backward of this forward follows, same dL/dlogits)
            accum = self.accum_steps > 1
            closing = not accum or self._micro == self.accum_steps - 1
            if accum:
                # a micro-step of an accumulation window (world_size > 1): the rank's row-weighted gradient and trailer are added to the accumulator; the closing
                # micro-step exchanges the ACCUMULATOR -- one all-reduce per window, on every rank -- and Adam divides by the row count summed over ranks and micro-steps
                from . import parallel
                _lib.check(L.qpn_train_backward_ex(hd, self._dlogits.data_ptr(), self.g.data_ptr(), float(B * BL), 1, stream))
                _lib.check(L.qpn_grad_accumulate(hd, self.acc.data_ptr(), self.g.data_ptr(), flat.numel() + 4, 1 if self._micro == 0 else 0, stream))
                if closing and multi:
                    parallel.exchange(self.acc, self.pg)
                    self.last_buckets = (0, 0)
                    L.qpn_train_profile_mark(hd, 9, stream)      # QPN_PG_ALLREDUCE
            elif multi:
                from .parallel import exchange_two_buckets
                first, count = C.c_int64(0), C.c_int64(0)
                if self._early is None:
                    self._early = torch.cuda.Stream(dev)
                # (opt-in, QPN_EXCHANGE_BUCKETS=2.  Measured with RCCL at one rank: the second call costs 18 us of stream time, 0.841 -> 0.859 ms a
                #  step; what it can hide at 8 ranks is a quarter of the bandwidth term of a 2.3 MB, latency-bound all-reduce -- DESIGN.md section 7)
                if self._two_buckets is None:
                    # How many collectives a step issues must not be a per-rank decision (environment and launch-plan knobs can differ per rank: a
                    # rank that sends one all-reduce while its peers send two deadlocks RCCL or corrupts the sum): the split is agreed ONCE, as the
                    # minimum over the ranks of "this rank wants and can do two buckets"; thereafter every rank issues two all-reduces over the SAME
                    # ranges in every step, whether or not its early range happened to be ready early in that step.
                    self._two_buckets = self._agree_two_buckets(L, hd, flat)
                # g <- n_r * grad_r with {n_r, flagged_r} appended; SUM over ranks; Adam divides by the summed row count on the device and skips the update on
                # EVERY rank when any rank's status word was set (2: the trailer leaves with the early bucket, before the backward's last launch could rewrite it)
                _lib.check(L.qpn_train_backward_ex(hd, self._dlogits.data_ptr(), self.g.data_ptr(), float(B * BL), 2 if self._two_buckets else 1, stream))
                # two buckets: the tail the side stream has finished already can go out under the layer backward (qpn_train_early_bucket)
                if self._two_buckets:
                    _lib.check(L.qpn_train_early_bucket(hd, C.byref(first), C.byref(count), self._early.cuda_stream))
                    if count.value == 0:      # nothing was finished early in this step (one stream: a profile is being taken): same two ranges, after the backward
                        first.value, count.value = self._two_buckets[0], self._two_buckets[1]
                        self._early.wait_stream(torch.cuda.current_stream(dev))
                exchange_two_buckets(self.g, first.value, count.value, self.pg, self._early if count.value else None)
                self.last_buckets = (first.value, count.value)       # (what the last step exchanged early; (0, 0): one exchange)
                L.qpn_train_profile_mark(hd, 9, stream)      # QPN_PG_ALLREDUCE (no-op unless a profile is being taken)
            else:
                _lib.check(L.qpn_train_backward(hd, self._dlogits.data_ptr(), self.g.data_ptr(), stream))
            clip = self.max_grad_norm
            gbuf = self.acc if accum else self.g
            den = gbuf.data_ptr() + 4 * flat.numel() if (multi or accum) else None
            if not closing:
                self._micro += 1                       # (no Adam launch: the window stays open)
            else:
                self.step_count += 1; self._micro = 0
                _lib.check(L.qpn_adam_step_avg(hd, flat.data_ptr(), gbuf.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), flat.numel(),
                                               self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, den, clip,
                                               self.ema.data_ptr() if self.ema is not None else None, self.ema_decay if self.ema is not None else 0.0, stream))
            if want_loss == "lagged":
                # this step's loss is copied out behind its kernels; what comes back is the PREVIOUS step's (None at the first step, or right after
                # flush_loss()): the stream is never drained, and a caller that sums losses over an interval and calls flush_loss() at its end has the same sum
                _lib.check(L.qpn_train_loss_enqueue(hd, stream))
                _lib.check(L.qpn_train_status_enqueue(hd, stream))
                valid = C.c_int(0)
                _lib.check(L.qpn_train_loss_collect(hd, 0, C.byref(loss), C.byref(valid)))
                if clip > 0.0 and valid.value:
                    self.last_grad_norm = self._collected_norm(L, hd)      # (it left the device in that loss's copy)
                return loss.value if valid.value else None
            if want_loss:
                _lib.check(L.qpn_train_loss(hd, C.byref(loss), stream))
                if clip > 0.0:
                    norm, nv = C.c_double(0.0), C.c_int(0)
                    _lib.check(L.qpn_train_grad_norm(hd, C.byref(norm), C.byref(nv), stream))
                    self.last_grad_norm = norm.value if nv.value else None
                _lib.check(L.qpn_train_status(hd, stream))   # (the stream has just been drained for the loss: in-step, like the reference)
            elif not capturing:
                _lib.check(L.qpn_train_status_enqueue(hd, stream))
        return loss.value if want_loss else None

    def _agree_two_buckets(self, L, hd, flat):
        """(first, count) of the early bucket if EVERY rank asked for two buckets (QPN_EXCHANGE_BUCKETS=2) and reports the same range, else False."""
        import torch.distributed as dist
        want = os.environ.get("QPN_EXCHANGE_BUCKETS", "1") == "2"
        first = int(L.qpn_train_early_first(hd)) if want else -1
        ok = want and first > 0
        if dist.is_initialized() and dist.get_world_size(self.pg) > 1:
            v = torch.tensor([first if ok else -1, -(first if ok else -1)], dtype=torch.int64, device=flat.device if dist.get_backend(self.pg) == "nccl" else "cpu")
            dist.all_reduce(v, op=dist.ReduceOp.MIN, group=self.pg)      # min(first) == max(first) > 0  <=>  every rank reports the same range
            ok = int(v[0]) > 0 and int(v[0]) == -int(v[1])
        return (first, flat.numel() - first + 4) if ok else False

    def flush_loss(self):
        """The loss of the last step(want_loss="lagged") (waits for that step), or None if it has been returned already."""
        L, hd = self.model._native(self.model._flat.device)
        loss, valid = C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_loss_collect(hd, 1, C.byref(loss), C.byref(valid)))
        if self.max_grad_norm > 0.0:
            self.last_grad_norm = self._collected_norm(L, hd) if valid.value else None
        return loss.value if valid.value else None

    @staticmethod
    def _collected_norm(L, hd):
        norm, nv = C.c_double(0.0), C.c_int(0)
        _lib.check(L.qpn_train_grad_norm_lagged(hd, C.byref(norm), C.byref(nv)))
        return norm.value if nv.value else None

    def check_status(self):
        """Raise what the device-side check of the last step(want_loss=False) found (see QPNet.check_status); the step count is set back to the
        updates the device actually applied (_rebase_step_count)."""
        try:
            self.model.check_status()
            teacher = self._distill[0] if self._distill is not None else None
            if teacher is not None and teacher._handle is not None:
                with torch.cuda.device(teacher._handle_dev):
                    self._teacher_check(_lib.lib(), _lib.lib().qpn_train_status_collect(teacher._handle))
        except _lib.QpnError as e:
            flat = getattr(self.model, "_flat", None)
            if e.code in (-4, -2) and flat is not None and flat.is_cuda:
                self._micro = 0                        # (an open accumulation window is abandoned)
                L, hd = self.model._native(flat.device)
                self._rebase_step_count(L, hd, flat.device, torch.cuda.current_stream(flat.device).cuda_stream, 0)
            raise

    def tensor_stats(self, weights="model"):
        """Per-tensor statistics of the latest Adam launch of this trainer: an ordered dict state_dict key -> {"grad_norm", "weight_norm", "update_norm",
        "update_ratio", "grad_absmax", "weight_absmax", "grad_nonfinite"}, in state_dict order (qpn_tensor_stats: two read-only launches over the buffers the step left).
        grad_*: the gradient that launch consumed, divided as the launch divided it -- with accum_steps > 1 the accumulator over its summed row count (the row-weighted
        mean gradient of the window), with world_size > 1 the exchanged buffer over its trailer -- before clipping; NaN / inf elements are counted in grad_nonfinite and
        left out of norm and maximum.  weight_*: the weights after the update (weights="ema": the averaged weights).  update_norm: the norm of what the launch subtracted
        from the tensor, rebuilt from m and v in the kernel's own fp32 expression and this tensor's group lr (float32(lr) * float32(lr_scale), over the bias correction);
        0 for a frozen tensor.  update_ratio = update_norm / weight_norm.
        A SYNCHRONOUS diagnostic call: it drains the current stream and reads the records back -- for a report every N steps, not for every step.  It changes nothing: weights,
        moments, losses, the status word and the applied-update count are what they are without it.  After a step the device skipped (a flagged chunk, a non-finite
        norm) m, v and, once the error has been raised, the step count are those of the last APPLIED update: the update fields describe that one, the gradient fields the
        gradient of the skipped step (grad_nonfinite says which tensor held the NaN).  `lr` is read now: call it before changing it for the next step.
        RuntimeError: before the first update, while an accumulation window is open (micro_step != 0: the accumulator holds part of a gradient) and on a capturing stream."""
        if weights not in ("model", "ema"):
            raise ValueError('tensor_stats: weights must be "model" or "ema", got %r' % (weights,))
        if weights == "ema" and self.ema_decay <= 0.0:
            raise RuntimeError('tensor_stats(weights="ema"): this trainer keeps no averaged weights (ema_decay is off)')
        model = self.model
        flat = getattr(model, "_flat", None)
        if self.step_count < 1 or self.m is None or self.g is None or flat is None or not flat.is_cuda or self.m.device != flat.device:
            raise RuntimeError("qpnet_amd.FusedTrainer.tensor_stats before the first update: there is no Adam launch to describe")
        if self._micro != 0:
            raise RuntimeError("qpnet_amd.FusedTrainer.tensor_stats while an accumulation window is open (micro_step = %d of %d): the accumulator holds part of a gradient"
                               % (self._micro, self.accum_steps))
        n = flat.numel()
        gbuf = self.acc if self.accum_steps > 1 else self.g
        den = gbuf.data_ptr() + 4 * n if (self.accum_steps > 1 or self.world > 1) else None
        n_tensors = len(model_params(model))
        if self._groups is not None:
            lrs = _tensor_lrs(n_tensors, self._groups.positions, self._group_values()[0])
        else:
            lrs = [self.lr] * n_tensors
        w = _ema_home(self.ema, flat) if weights == "ema" else flat
        return _tensor_stats("FusedTrainer", model, w, gbuf, den, self.m, self.v, self.step_count, self.betas, self.eps, lrs)

    def forward_loss(self, x, h, t, d, blength, maxd=None, weights="model"):
        """forward + mean CE only (validation, reference qpnet_validate.py:409-430).  weights="ema": of the averaged weights (the forward reads the flat vector
        it is handed at call time; the live weights are not touched); raises when averaging is off."""
        if weights not in ("model", "ema"):
            raise ValueError('forward_loss: weights must be "model" or "ema", got %r' % (weights,))
        if weights == "ema" and self.ema_decay <= 0.0:
            raise RuntimeError('forward_loss(weights="ema"): this trainer keeps no averaged weights (ema_decay is off)')
        model = self.model
        dev = x.device
        L, hd = model._native(dev)
        flat = ensure_flat(model, dev)
        if weights == "ema":
            self.ema = _ema_home(self.ema, flat)
            flat = self.ema
        join_staged(x, dev, h, t, d)                 # (run_validate feeds staged batches: the copy stream must be joined before anything reads them)
        x = self._norm(x, torch.int64, dev); t = self._norm(t, torch.int64, dev)
        h = self._norm(h, torch.float32, dev); d = self._norm(d, torch.float32, dev)
        BL = int(blength[0])
        if maxd is None:
            maxd = int(torch.max(d.ceil()))
        B, T = x.shape
        logits = torch.empty((B, BL, model.n_quantize), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        loss = C.c_double(0.0)
        with torch.cuda.device(dev):
            _lib.check(L.qpn_train_forward_loss(hd, flat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd,
                                                x.data_ptr(), h.data_ptr(), d.data_ptr(), t.data_ptr(), t.shape[1],
                                                logits.data_ptr(), 0, None, stream))
            _lib.check(L.qpn_train_loss(hd, C.byref(loss), stream))
            _lib.check(L.qpn_train_status(hd, stream))
        return loss.value

    def score(self, x, h, t, d, blength, maxd=None, weights="model"):
        """forward + per-sample records of the chunk's last `blength` targets (score_logits): arguments and checks of forward_loss, -> Score of (B, BL)
        tensors.  A target outside [0, n_quantize) is not an error here: its record says nll = +inf, rank = n_quantize."""
        if weights not in ("model", "ema"):
            raise ValueError('score: weights must be "model" or "ema", got %r' % (weights,))
        if weights == "ema" and self.ema_decay <= 0.0:
            raise RuntimeError('score(weights="ema"): this trainer keeps no averaged weights (ema_decay is off)')
        model = self.model
        dev = x.device
        L, hd = model._native(dev)
        flat = ensure_flat(model, dev)
        if weights == "ema":
            self.ema = _ema_home(self.ema, flat)
            flat = self.ema
        join_staged(x, dev, h, t, d)
        x = self._norm(x, torch.int64, dev); t = self._norm(t, torch.int64, dev)
        h = self._norm(h, torch.float32, dev); d = self._norm(d, torch.float32, dev)
        BL = int(blength[0])
        if maxd is None:
            maxd = int(torch.max(d.ceil()))
        B, T = x.shape
        logits = torch.empty((B, BL, model.n_quantize), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(L.qpn_train_forward(hd, flat.data_ptr(), B, T, h.shape[2], d.shape[1], BL, maxd,
                                           x.data_ptr(), h.data_ptr(), d.data_ptr(), logits.data_ptr(), stream))
            s = score_logits(logits, t)
            _lib.check(L.qpn_train_status(hd, stream))
        return s

    # ---- optimizer-state interface (checkpoints: loaders.save_checkpoint(dir, model, trainer, it))
    def _hyper(self):
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.wd)

    def _state_groups(self):
        """the groups state_dict() writes: the default group when it holds a tensor, then every entry that is not frozen"""
        lrs, wds = self._group_values()
        return [(g, dict(lr=lrs[g], betas=self.betas, eps=self.eps, weight_decay=wds[g]), ps) for g, ps in enumerate(self._groups.positions) if ps]

    def state_dict(self):
        if self._groups is not None:
            return adam_state_to_torch(self.model, self.m, self.v, self.step_count, None, [(hyp, ps) for _, hyp, ps in self._state_groups()])
        return adam_state_to_torch(self.model, self.m, self.v, self.step_count, self._hyper())

    def ema_state_dict(self):
        """the averaged weights under the model's state_dict() keys, shapes and order ({} with averaging off): load it into a model to decode with the average."""
        return _ema_to_state_dict(self.model, self.ema) if self.ema_decay > 0.0 else {}

    def load_ema(self, sd):
        """restore the average from an ema_state_dict(); None: seed it from the current weights at the next step.  Works on a CPU model (a checkpoint is loaded
        before the model has seen the device): the tensor moves at the first step, as the moments do."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("load_ema: this trainer keeps no averaged weights (ema_decay is off)")
        self.ema = None if sd is None else _ema_from_state_dict(self.model, sd)

    def load_state_dict(self, sd):
        params = list(self.model.parameters())
        flat = getattr(self.model, "_flat", None)
        if flat is None or flat.device != params[0].device:
            flat = torch.cat([p.detach().reshape(-1).float() for p in params])
        if self._groups is not None:
            # lr_scale and the entries' own weight decays are this trainer's settings.  Of the file's values: betas and eps; the base lr, from the first group
            # whose scale is not 0 (the file holds lr * lr_scale; with every scale 0 the trainer's lr stays); the trainer's weight_decay, from the default group
            # when the file has it (it is written first) -- as the load without groups takes lr and weight_decay from the file's one group
            groups = self._state_groups()
            self.m, self.v, self.step_count, hypers = adam_state_from_torch(self.model, sd, flat, [ps for _, _, ps in groups])
            for (g, _, _), hyper in zip(groups, hypers):
                if "lr" in hyper and self._group_scales[g] > 0.0:
                    self.lr = hyper["lr"] if g == 0 else hyper["lr"] / self._group_scales[g]
                    break
            if groups[0][0] == 0:
                self.wd = hypers[0].get("weight_decay", self.wd)
            self.betas = tuple(hypers[0].get("betas", self.betas)); self.eps = hypers[0].get("eps", self.eps)
            return
        self.m, self.v, self.step_count, hyper = adam_state_from_torch(self.model, sd, flat)
        self.lr = hyper.get("lr", self.lr); self.betas = tuple(hyper.get("betas", self.betas))
        self.eps = hyper.get("eps", self.eps); self.wd = hyper.get("weight_decay", self.wd)
