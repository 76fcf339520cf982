"""Emit tests/golden/launch_sequences.json: the ordered ``icm_*`` entry-point calls of the codec and of a training step.

Run on a GPU against the code whose launch order is to be pinned (the fixture was written from the slice loops as they
stood before they shared one prologue, one per-slice coding step and one quantiser object);
tests/test_gpu_launch_sequences.py runs every case again and wants the same calls in the same order.

A case runs once to warm up (weights packed, tables built, the step table uploaded), then once more with ``_lib.lib``
replaced by a recorder.  The cases:

  codec  compress + decompress of a 1x3x64x64 image (a 4x4 latent, the smallest the models take), cnn and stf, both forms
         of the slice loop, without a step, with ``qstep=5`` and with a non-uniform 4x4 quality map.  cnn's 5 tail slices
         are one batch; stf's 6 exceed ``MAX_GROUP // 2`` and run as two
  train  train-mode forward + backward with injected noise (stf: and DropPath scales), cnn and stf in both forms at
         1x3x64x64, stf6 (the zigzag loop) at 1x3x128x128

  {"names": [entry points], "cases": {case id: [index into names, ...]}}

Usage: python tests/golden/make_launch_sequences.py"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "launch_sequences.json")
STATE_DICTS = {"cnn": W.make_wacnn_state_dict, "stf": W.make_stf_state_dict, "stf6": W.make_stf6_state_dict}
LATENT = {"cnn": 320, "stf": 384, "stf6": 384}
QMAP = np.array([-16, -3, 0, 5, 32], dtype=np.int8)[(3 * np.arange(4)[:, None] + np.arange(4)[None, :]) % 5]
QUALITY = {"none": {}, "qstep5": {"qstep": 5}, "qmap": {"qmap": QMAP}}


def _cases():
    out = []
    for quality in QUALITY:
        for arch in ("cnn", "stf"):
            for split in (True, False):
                out.append({"kind": "codec", "arch": arch, "split": split, "quality": quality, "side": 64})
    for arch in ("cnn", "stf"):
        for split in (True, False):
            out.append({"kind": "train", "arch": arch, "split": split, "quality": "none", "side": 64})
    out.append({"kind": "train", "arch": "stf6", "split": None, "quality": "none", "side": 128})
    for c in out:
        form = {True: "split_slices", False: "unsplit", None: "zigzag"}[c["split"]]
        c["id"] = "-".join([c["kind"], c["arch"], form] + ([c["quality"]] if c["kind"] == "codec" else []))
    return out


CASES = _cases()


class RecordingLib:
    """the real library, with the names of the ``icm_*`` entry points called kept in order"""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("icm_"):
            return fn

        def recorded(*a):
            self.names.append(name)
            return fn(*a)
        return recorded


def _net(nets, arch, train):
    """one model per (arch, mode), shared by the cases"""
    if (arch, train) not in nets:
        from icm_amd.zoo import models
        m = models[arch]()
        m.load_state_dict(STATE_DICTS[arch]())
        m = m.to(DEV)
        if train:
            m.train()
        else:
            m.eval()
            m.update(force=True)
        nets[(arch, train)] = m
    return nets[(arch, train)]


def _injected(arch, side):
    from icm_amd import models as M
    key = f"launchseq.{arch}"
    noise = {"z": W._u(key + ".nz", (1, 192, side // 64, side // 64), -0.5, 0.5)}
    if arch == "stf6":
        noise["y"] = W._u(key + ".ny", (1, 24, 64, side // 32, side // 32), -0.5, 0.5)
    else:
        noise["y"] = W._u(key + ".ny", (1, LATENT[arch], side // 16, side // 16), -0.5, 0.5)
    if arch == "cnn":
        return (noise,)
    rates = M.stf6_drop_path_rates() if arch == "stf6" else M.stf_drop_path_rates()
    drops = {name: (W._u(f"{key}.dp.{name}", (2, 1), 0.0, 1.0) < 1.0 - r).float() / (1.0 - r) for name, r in rates.items()
             if r > 0}
    assert any(float(d.min()) == 0.0 for d in drops.values()), "no residual branch is dropped"
    return noise, drops


def prepare(case, nets):
    """the case as a callable that returns what it computed: {"strings", "x_hat"} of the codec, {"x_hat", "y_lik",
    "z_lik", "grads": {name: gradient}} of a training step"""
    arch, side = case["arch"], case["side"]
    x = W._u("launchseq.x", (1, 3, side, side), 0.0, 1.0).to(DEV)
    if case["kind"] == "codec":
        m, q = _net(nets, arch, False), QUALITY[case["quality"]]

        def codec():
            enc = m.compress(x, **q)
            dec = m.decompress(enc["strings"], enc["shape"], **q)
            return {"strings": enc["strings"], "x_hat": dec["x_hat"]}
        return codec
    from icm_amd.losses import RateDistortionLoss
    m, injected = _net(nets, arch, True), _injected(arch, side)
    crit = RateDistortionLoss(0.0067)

    def train():
        m.zero_grad(set_to_none=True)
        m.inject_noise(*injected)
        out = m(x)
        crit(out, x)["loss"].backward()
        torch.cuda.synchronize()
        return {"x_hat": out["x_hat"], "y_lik": out["likelihoods"]["y"], "z_lik": out["likelihoods"]["z"],
                "grads": {n: p.grad for n, p in m.named_parameters() if p.grad is not None}}
    return train


def sequence(case, nets, setattr_):
    """the entry points one run of the case calls, in order.  ``setattr_(object, name, value)`` makes the two
    replacements (the form of the slice loop, the library); undoing them is the caller's business"""
    from icm_amd import _lib
    from icm_amd import models as M
    if case["split"] is not None:
        setattr_(M, "SLICE_SPLIT", case["split"])
    run = prepare(case, nets)
    run()
    rec = RecordingLib(_lib.lib())
    setattr_(_lib, "lib", lambda: rec)
    run()
    return rec.names


def main():
    from icm_amd import _lib
    from icm_amd import models as M
    nets, names, cases = {}, {}, {}
    for case in CASES:
        saved = (M.SLICE_SPLIT, _lib.lib)
        try:
            seq = sequence(case, nets, setattr)
        finally:
            M.SLICE_SPLIT, _lib.lib = saved
        cases[case["id"]] = [names.setdefault(n, len(names)) for n in seq]
        print(f"{case['id']}: {len(seq)} calls, {len(set(seq))} entry points")
    with open(FIXTURE, "w") as fh:
        json.dump({"names": list(names), "cases": cases}, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {os.path.basename(FIXTURE)}: {len(names)} names, {len(cases)} cases, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
