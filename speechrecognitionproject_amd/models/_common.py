"""Evaluation helpers shared by every model plugin — same behaviour as the reference's
per-module copies (e.g. models/model_mfcc_bgru.py:39-82), including its quirks:
``total += batchsize`` over-counts a short last batch (:51), and ``class_accuracy`` iterates
``range(batchsize)`` (:67), so it needs a dataset length divisible by ``batchsize``."""
import torch
from torch.utils.data import DataLoader

LABELS = ['yes', 'no', 'up', 'down', 'left', 'right', 'on', 'off', 'stop', 'go', 'unknown', 'silence']
DEVICE = torch.device('cuda' if torch.cuda.is_available() else 'cpu')


def check_specaug(specaug, T, F):
    """The constructor argument ``specaug`` of a plugin whose network reads [T, F] clips, as a checked
    ``features.SpecAugPolicy``, or None.  Accepts a policy or a sequence (W, NF, f_max, NT, t_max[, p[, fill]])."""
    if specaug is None:
        return None
    from .. import features
    return features.as_specaug_policy(specaug).check_shape(T, F)


def apply_specaug(net, feat, specaug_params=None):
    """SpecAugment for the plugins (``Network(specaug=...)``): masks and warps ``feat``, the time-major feature
    tensor [B, T, F] the network is about to read, IN PLACE and returns it.  Training mode only — ``eval()`` and
    ``specaug=None`` leave ``feat`` untouched, bit for bit.  The parameters are ``specaug_params`` (int32 [B, P],
    for tests) or a fresh device draw into one persistent buffer per (device, batch size), kept for the module's
    life as the VTLP factors are: a captured step of the full batch keeps its address while a short last batch
    runs eagerly on another.  ``net.last_specaug`` holds the parameters of the last augmented batch."""
    pol = net.specaug
    if pol is None:
        if specaug_params is not None:
            raise ValueError("specaug_params needs a network built with specaug=... (NF, NT and the fill come from it)")
        return feat
    if not net.training:
        return feat
    from .. import features
    B, T, F = feat.shape
    if specaug_params is None:
        key = (feat.device.index, B)
        buf = net._specaug_bufs.get(key)
        if buf is None:
            buf = net._specaug_bufs[key] = torch.empty((B, pol.n_params), device=feat.device, dtype=torch.int32)
        specaug_params = features.specaug_draw(B, T, F, pol, out=buf)
    elif not torch.is_tensor(specaug_params):
        specaug_params = torch.as_tensor(specaug_params, dtype=torch.int32).to(feat.device)
    net.last_specaug = specaug_params
    return features.spec_augment(feat, specaug_params, pol, time_major=True, out=feat)


def accuracy(model, dataset, filename, batchsize=2):
    """Overall accuracy (%) on ``dataset``; appends it as one line to ``filename``."""
    total, correct = 0, 0
    model.eval()
    dataloader = DataLoader(dataset, batch_size=batchsize, drop_last=False)
    with torch.no_grad():
        for batch in dataloader:
            outputs = model(batch['audio'])
            _, predicted = torch.max(outputs.data, 1)
            total += batchsize
            correct += (predicted == batch['label'].to(outputs.device)).sum().item()
    with open(filename, 'a') as f:
        f.write(str(100 * correct / float(total)) + '\n')
    model.train()
    return 100 * correct / float(total)


def class_accuracy(model, dataset, filename, batchsize=2):
    """Per-class accuracy; overwrites ``filename`` with 12 lines."""
    class_correct = [0.0] * 12
    class_total = [0.0] * 12
    model.eval()
    dataloader = DataLoader(dataset, batch_size=batchsize, drop_last=False)
    with torch.no_grad():
        for batch in dataloader:
            outputs = model(batch['audio'])
            _, predicted = torch.max(outputs.data, 1)
            c = (predicted == batch['label'].to(outputs.device)).squeeze()
            for i in range(batchsize):
                label = batch['label'][i]
                class_correct[label] += c[i].item()
                class_total[label] += 1
    with open(filename, 'w') as f:
        for i in range(12):
            f.write('Accuracy of %5s : %2d %%' % (LABELS[i], 100 * class_correct[i] / class_total[i]) + '\n')
    model.train()
