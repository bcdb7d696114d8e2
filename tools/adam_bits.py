"""The optimiser step of this tree's library against another build's (the parent commit's), as bit patterns.

    python tools/adam_bits.py [--parent build_variants/libqpnet_parent.so]

One fixed input set, run in a fresh process per library (QPN_LIB selects it):
  A. qpn_adam_step_avg on hand-made buffers: n = 2051 and TINY's parameter count, all 8 kernel instances (clip x averaged weights x groups), without and with a
     denominator buffer {3, 0, 0, 0}, three steps each.  Kept: w, m, v, e after every step, the norm, qpn_train_status' return, the applied-update count.
  B. qpn_train_step_acc on TINY chunks: loss modes 0 / 1 / 2, windows of 1 and 2, three updates each, clipping and averaging on.  Kept: every returned double
     (loss, norm) and flag, w, m, v, e and the accumulator at the end, the status return, the applied-update count.
Part A is deterministic and must be equal bit for bit (int32 views); the exit code says so.  Part B runs a forward and a backward whose float atomics make two runs
of ONE library differ in the last bits, so the other build is run twice: integers and flags must be equal, the floats are reported as the largest difference
between the two builds next to the largest difference between the other build's own two runs."""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
FROZEN = -1


def _child(out_path):
    import torch
    from qpnet_amd import _lib, synth
    from qpnet_amd.config import TINY
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}

    def to(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def applied(hp):
        n = C.c_int64(-1)
        _lib.check(L.qpn_train_applied_updates(hp, C.byref(n), stream))
        return int(n.value)

    # ---- A
    hp = C.c_void_p()
    _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
    lrs, wds = [1e-3, 3e-4, 2e-2], [0.0, 1e-2, 1e-3]
    warm = [torch.full((8,), x, dtype=torch.float32, device=dev) for x in (0.1, 0.01, 0.0, 0.0)]      # (a clipping call creates the training state: the status word, the count)
    _lib.check(L.qpn_adam_step_avg(hp, warm[0].data_ptr(), warm[1].data_ptr(), warm[2].data_ptr(), warm[3].data_ptr(), 8, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, 1.0, None, 0.0, stream))
    for n in (2051, TINY.n_params):
        ends = [300, 1000, 1030, 2051] if n == 2051 else [n // 7, n // 3, n // 3 + 30, n]
        groups = [0, FROZEN, 1, 2]
        rs = np.random.RandomState(n)
        w0, m0 = (rs.standard_normal(n) * 0.1).astype(F), (rs.standard_normal(n) * 0.003).astype(F)
        v0, e0 = ((rs.standard_normal(n) * 0.01) ** 2 * 0.5).astype(F), (rs.standard_normal(n) * 0.1).astype(F)
        gs = [(rs.standard_normal(n) * 0.01).astype(F) for _ in range(3)]
        max_norm = 0.25 * float(np.sqrt((gs[0].astype(np.float64) ** 2).sum()))
        for clip, ema, grp, den in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            key = "A/n%d/clip%d_ema%d_grp%d_den%d" % (n, clip, ema, grp, den)
            if grp:
                _lib.check(L.qpn_adam_groups(hp, 3, (C.c_float * 3)(*lrs), (C.c_float * 3)(*wds), 4, (C.c_int64 * 4)(*ends), (C.c_int32 * 4)(*groups), stream))
            else:
                _lib.check(L.qpn_adam_groups(hp, 0, None, None, 0, None, None, None))
            w, m, v, e = to(w0), to(m0), to(v0), to(e0)
            dden = torch.tensor([3.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev) if den else None
            for k in range(3):
                g = to(gs[k] * F(3.0) if den else gs[k])
                _lib.check(L.qpn_adam_step_avg(hp, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, k + 1, 1e-3, 0.9, 0.999, 1e-8, 1e-3,
                                               dden.data_ptr() if den else None, max_norm if clip else 0.0, e.data_ptr() if ema else None, 0.9 if ema else 0.0, stream))
                norm, nv = C.c_double(0.0), C.c_int(0)
                _lib.check(L.qpn_train_grad_norm(hp, C.byref(norm), C.byref(nv), stream))
                for name, t in zip("wmve", (w, m, v, e)):
                    out["%s/step%d/%s" % (key, k, name)] = t.cpu().numpy()
                out["%s/step%d/norm" % (key, k)] = np.array([norm.value], np.float64)
                out["%s/step%d/ints" % (key, k)] = np.array([nv.value, L.qpn_train_status(hp, stream), applied(hp)], np.int64)
    L.qpn_destroy(hp)

    # ---- B
    N = TINY.n_params
    w0 = synth.make_weights(TINY, 3)
    chunks = [synth.train_inputs(TINY, bl, 900 + i, 30000) for i, bl in enumerate([300, 410, 350, 280, 300, 410])]
    for mode, K in itertools.product((0, 1, 2), (1, 2)):
        key = "B/mode%d_window%d" % (mode, K)
        hp = C.c_void_p()
        _lib.check(L.qpn_create(C.byref(_lib.make_config(TINY)), C.byref(hp)))
        flat, ema = to(w0), to(w0)
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        g = torch.zeros(N + 4, dtype=torch.float32, device=dev)
        acc = torch.full((N + 4,), float("nan"), dtype=torch.float32, device=dev)
        doubles, ints = [], []
        for call in range(3 * K):
            x, h, t, d, b = chunks[call]
            xt, ht, tt, dt = to(x), to(h), to(t), to(d)
            B, BL = x.shape[0], int(b[0])
            logits = torch.empty((B, BL, TINY.n_quantize), dtype=torch.float32, device=dev)
            dlogits = torch.empty_like(logits)
            loss, valid, norm = C.c_double(0.0), C.c_int(0), C.c_double(0.0)
            rc = L.qpn_train_step_acc(hp, flat.data_ptr(), B, x.shape[1], ht.shape[2], dt.shape[1], BL, int(np.ceil(d).max()), xt.data_ptr(), ht.data_ptr(), dt.data_ptr(),
                                      tt.data_ptr(), tt.shape[1], logits.data_ptr(), dlogits.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N,
                                      call // K + 1, 1e-4, 0.9, 0.999, 1e-8, 0.0, mode, C.byref(loss), C.byref(valid), 0.05, C.byref(norm),
                                      ema.data_ptr(), 0.9, acc.data_ptr() if K > 1 else None, call % K, K, stream)
            doubles += [loss.value, norm.value]
            ints += [rc, valid.value]
        if mode == 1:
            loss, valid, norm, nv = C.c_double(0.0), C.c_int(0), C.c_double(0.0), C.c_int(0)
            _lib.check(L.qpn_train_loss_collect(hp, 1, C.byref(loss), C.byref(valid)))
            _lib.check(L.qpn_train_grad_norm_lagged(hp, C.byref(norm), C.byref(nv)))
            doubles += [loss.value, norm.value]
            ints += [valid.value, nv.value]
        ints += [L.qpn_train_status(hp, stream), applied(hp)]
        for name, t in zip(("w", "m", "v", "e"), (flat, m, v, ema)):
            out["%s/%s" % (key, name)] = t.cpu().numpy()
        if K > 1:
            out[key + "/acc"] = acc.cpu().numpy()
        out[key + "/doubles"] = np.array(doubles, np.float64)
        out[key + "/ints"] = np.array(ints, np.int64)
        L.qpn_destroy(hp)
    np.savez(out_path, **out)


def _run(lib, out_path):
    env = dict(os.environ)
    if lib:
        env["QPN_LIB"] = os.path.abspath(lib)
    else:
        env.pop("QPN_LIB", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out_path], check=True, env=env, cwd=ROOT, timeout=600)
    return dict(np.load(out_path))


def _bits(a):
    return a.view(np.int32) if a.dtype in (np.float32, np.float64) else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "build_variants", "libqpnet_parent.so"))
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return _child(args.child)
    with tempfile.TemporaryDirectory() as tmp:
        par = _run(args.parent, os.path.join(tmp, "parent.npz"))
        new = _run(None, os.path.join(tmp, "new.npz"))
        par2 = _run(args.parent, os.path.join(tmp, "parent2.npz"))
    assert par.keys() == new.keys() == par2.keys()
    a_keys = [k for k in par if k.startswith("A/")]
    a_diff = [k for k in a_keys if not np.array_equal(_bits(par[k]), _bits(new[k]))]
    b_int = [k for k in par if k.startswith("B/") and k.endswith("/ints")]
    b_int_diff = [k for k in b_int if not np.array_equal(par[k], new[k])]
    b_flt = [k for k in par if k.startswith("B/") and not k.endswith("/ints")]

    def spread(x, y):
        rows = {}
        for k in b_flt:
            a, b = x[k].astype(np.float64), y[k].astype(np.float64)
            same = np.array_equal(_bits(x[k]), _bits(y[k]))
            rows[k] = {"bit_equal": bool(same), "max_abs_diff": 0.0 if same else float(np.nanmax(np.abs(a - b)))}
        return rows
    res = {"what": "optimiser step, this tree's library against " + os.path.relpath(args.parent, ROOT),
           "A_arrays": len(a_keys), "A_arrays_differing": a_diff, "B_int_arrays": len(b_int), "B_int_arrays_differing": b_int_diff,
           "A_cases": len({k.rsplit("/", 2)[0] for k in a_keys}), "B_new_vs_parent": spread(par, new), "B_parent_vs_parent": spread(par, par2)}
    print(json.dumps(res))
    sys.exit(1 if a_diff or b_int_diff else 0)


if __name__ == "__main__":
    main()
