"""Generate tests/golden/resnet_dconv_golden.npz FROM THE REFERENCE ITSELF (models/model_resnet_dconv.py).

Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_resnet_dconv_golden.py [seed]

The reference is imported read-only.  The output is data only: the clips, and what the reference computes on
them with the seeded weights (``OM.seeded_state_dict(net, 0)``; the 25.9 M weights themselves are never stored).

Clips are B = 2 of white noise, rint(N(0, 3000)) — not ``synthetic_clips``, whose silent and periodic stretches
give max-pool near-ties on which the reference's own float32 and float64 gradients of ``dilation.conv3.weight``
differ by 17 %.  Two records, each from the reference run in float32 AND in float64:

* ``ev_*``: eval mode (BatchNorm on its running statistics): logits, loss, per parameter 64 sampled gradient
  entries plus the largest-|g| one, and the sampled first-step Adam deltas (lr 1e-4) of the float32 run.
* ``tr_*``: train mode: logits, loss, the BatchNorm running statistics after the forward, the same sampled
  gradients.  A single ReLU sign flip between float32 and float64 moves whole gradient tensors here, so the
  generator asserts that on the chosen seed the reference's OWN float32 gradients stay within 1.25e-2 of its
  float64 ones (normwise over the sampled entries, per tensor) and records that figure (``tr_ref32_norm_err``).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.dont_write_bytecode = True   # the reference tree is read-only: no __pycache__ left behind
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import models as OM                     # noqa: E402
from resnet_dconv_oracle import white_noise_clips   # noqa: E402

N_SAMPLED = 64
SEED = int(sys.argv[1]) if len(sys.argv) > 1 else 12
REF32_NORM_MAX = 1.25e-2


def sample_idx(g64, seed=99):
    """64 sampled flat indices (all of them for tensors of <= 64 entries) plus the largest-|g| entry."""
    flat = g64.reshape(-1)
    if flat.numel() <= N_SAMPLED:
        idx = np.arange(flat.numel())
    else:
        idx = np.sort(np.random.default_rng(seed).choice(flat.numel(), N_SAMPLED, replace=False))
    return np.concatenate([idx, [int(flat.abs().argmax())]]).astype(np.int64)


def run(R, sd, x, labels, dtype, train_mode, adam):
    net = R.Network()
    net.load_state_dict(sd)
    net = net.to(dtype)
    net.train(train_mode)
    params = dict(net.named_parameters())
    before = {k: v.detach().clone() for k, v in params.items()}
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    opt.zero_grad()
    out = net(torch.from_numpy(x).to(dtype))
    loss = torch.nn.CrossEntropyLoss()(out, torch.from_numpy(labels))
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in params.items()}
    delta = None
    if adam:
        opt.step()
        delta = {k: (v.detach() - before[k]) for k, v in params.items()}
    stats = {k: v.detach().clone() for k, v in net.state_dict().items()
             if k.endswith("running_mean") or k.endswith("running_var")}
    return out.detach(), loss.detach(), grads, delta, stats


def main():
    sys.path.insert(0, REF)
    from models import model_resnet_dconv as R
    torch.manual_seed(0)
    x, labels = white_noise_clips(2, SEED)
    proto = R.Network()
    sd = OM.seeded_state_dict(proto, 0)
    rec = {"pcm": x, "labels": labels, "seed": np.int64(SEED),
           "sd_keys": np.array(list(proto.state_dict().keys())),
           "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in proto.state_dict().values()]),
           "names": np.array([k for k, _ in proto.named_parameters()])}
    for tag, train_mode in (("ev", False), ("tr", True)):
        o32, l32, g32, d32, s32 = run(R, sd, x, labels, torch.float32, train_mode, adam=not train_mode)
        o64, l64, g64, _, s64 = run(R, sd, x, labels, torch.float64, train_mode, adam=False)
        rec[tag + "_logits32"], rec[tag + "_logits64"] = o32.numpy(), o64.numpy()
        rec[tag + "_loss32"], rec[tag + "_loss64"] = np.float32(l32.item()), np.float64(l64.item())
        worst_norm = worst_max = 0.0
        for k in g64:
            idx = sample_idx(g64[k])
            a = g32[k].reshape(-1).numpy()[idx]
            b = g64[k].reshape(-1).numpy()[idx]
            rec["%s_gidx__%s" % (tag, k)] = idx
            rec["%s_g32__%s" % (tag, k)] = a
            rec["%s_g64__%s" % (tag, k)] = b
            if d32 is not None:
                rec["%s_dval__%s" % (tag, k)] = d32[k].reshape(-1).numpy()[idx]
            worst_norm = max(worst_norm, float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)))
            worst_max = max(worst_max, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)))
        rec[tag + "_ref32_norm_err"], rec[tag + "_ref32_max_err"] = np.float64(worst_norm), np.float64(worst_max)
        lerr = float(np.abs(o32.numpy() - o64.numpy()).max() / np.abs(o64.numpy()).max())
        print("%s: reference float32 vs float64: logits %.2e, loss %.2e, gradients normwise %.2e, max-norm %.2e"
              % (tag, lerr, abs(l32.item() - l64.item()), worst_norm, worst_max))
        if train_mode:
            assert worst_norm <= REF32_NORM_MAX, "seed %d: the reference's own float32 train-mode gradients are %.3g " \
                "off its float64 ones; choose another seed" % (SEED, worst_norm)
            for k in s64:
                rec["tr_stat32__" + k], rec["tr_stat64__" + k] = s32[k].numpy(), s64[k].numpy()
    out = os.path.join(HERE, "resnet_dconv_golden.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
