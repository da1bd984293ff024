"""Shared by tests/test_bigru_last_group_gpu.py and run by it as a subprocess (the grouping switch SRK_GEMM_GROUP is
read once per process): one BiGRU layer, H = 512, forward_last or last_step(forward(x)[0]) with the loss
sum(y * g), every result as a tensor.

    python bigru_group_worker.py IN B T out.pt     # forward_last under the process's environment -> torch.save
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

H = 512
GROUP_RECORD = "gemm_p32_group<TN>"


def inputs(IN, B, T, seed=11):
    """(state_dict, x, g) in float32 from a seeded generator."""
    from speechrecognitionproject_amd import nn as snn
    gen = torch.Generator().manual_seed(seed)
    gru = snn.BiGRU(IN, H, num_layers=1)
    sd = {k: torch.empty(v.shape).uniform_(-H ** -0.5, H ** -0.5, generator=gen) for k, v in gru.state_dict().items()}
    return sd, torch.randn(B, T, IN, generator=gen), torch.randn(B, 2 * H, generator=gen)


def device_gru(IN, sd):
    from speechrecognitionproject_amd import nn as snn
    gru = snn.BiGRU(IN, H, num_layers=1).cuda()
    gru.load_state_dict(sd)
    return gru


def run(gru, x, g, last):
    """{"y", "dx", "d<parameter>"} of forward_last (last) or last_step(forward(x)[0])."""
    from speechrecognitionproject_amd import nn as snn
    for p in gru.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(True)
    y = gru.forward_last(xg) if last else snn.last_step(gru(xg)[0])
    (y * g.cuda()).sum().backward()
    torch.cuda.synchronize()
    out = {"y": y.detach().clone(), "dx": xg.grad.detach().clone()}
    out.update({"d" + k: p.grad.detach().clone() for k, p in gru.named_parameters()})
    return out


def main(argv):
    IN, B, T = (int(a) for a in argv[:3])
    sd, x, g = inputs(IN, B, T)
    res = run(device_gru(IN, sd), x, g, True)
    torch.save({k: v.cpu() for k, v in res.items()}, argv[3])


if __name__ == "__main__":
    main(sys.argv[1:])
