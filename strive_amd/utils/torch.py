"""Checkpoint and small tensor helpers under the reference's names (reference src/utils/torch.py:9-71).

A checkpoint is the dictionary ``{'model', 'optim', 'epoch', 'min_val_loss'}`` written by ``torch.save``: a file written by
``save_state`` here loads with the reference's ``load_state`` and the other way round.  (Inside this package ``import torch``
is the absolute import of PyTorch; the module is reached as ``strive_amd.utils.torch``.)
"""
import os

import numpy as np
import torch

WARN_MISSING = 'WARNING: The following keys could not be found in the given state dict - ignoring...'
WARN_UNEXPECTED = 'WARNING: The following keys were found in the given state dict but not in the current model - ignoring...'


def c2c(tensor):
    """Tensor -> numpy array on the host, detached."""
    return tensor.detach().cpu().numpy()


def get_device():
    return torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')


def count_params(model):
    """Number of trainable scalars."""
    return sum(int(np.prod(p.size())) for p in model.parameters() if p.requires_grad)


def _top_level_filter(keys, ignore_keys):
    """Entries whose first dotted component is not among ``ignore_keys`` (None keeps everything)."""
    if ignore_keys is None:
        return list(keys)
    return [k for k in keys if k.split('.')[0] not in ignore_keys]


def save_state(file_out, model, optimizer, cur_epoch=0, min_val_loss=float('Inf'), ignore_keys=None):
    state = model.state_dict()
    state = {k: state[k] for k in _top_level_filter(state.keys(), ignore_keys)}
    torch.save({'model': state, 'optim': optimizer.state_dict(), 'epoch': cur_epoch, 'min_val_loss': min_val_loss}, file_out)


def load_state(load_path, model, optimizer=None, map_location=None, ignore_keys=None):
    """Non-strict load of ``checkpoint['model']`` into ``model`` (and of ``checkpoint['optim']`` into ``optimizer`` when one is
    given); sub-modules named in ``ignore_keys`` are neither loaded nor reported.  Returns ``(epoch, min_val_loss)``."""
    if not os.path.exists(load_path):
        print('Could not find checkpoint at path ' + load_path)
    ckpt = torch.load(load_path, map_location=map_location)
    state = ckpt['model']
    state = {k: state[k] for k in _top_level_filter(state.keys(), ignore_keys)}
    missing, unexpected = model.load_state_dict(state, strict=False)
    missing, unexpected = _top_level_filter(missing, ignore_keys), _top_level_filter(unexpected, ignore_keys)
    if len(missing) > 0:
        print(WARN_MISSING)
        print(missing)
    if len(unexpected) > 0:
        print(WARN_UNEXPECTED)
        print(unexpected)
    if optimizer is not None:
        optimizer.load_state_dict(ckpt['optim'])
    return ckpt['epoch'], ckpt['min_val_loss']


def calc_conv_out(in_size, kernel_size, stride, padding_size=0):
    return int(((in_size - kernel_size - 2 * padding_size) // stride) + 1)


def compute_kl_weight(cur_epoch, end_epoch, final_kl_weight):
    """Linear annealing from 0 at epoch 0 to ``final_kl_weight`` at ``end_epoch``."""
    return min(1.0, float(cur_epoch) / end_epoch) * final_kl_weight


def tensor_clamp(x, xmin, xmax):
    """Clamp with tensor bounds."""
    return torch.max(torch.min(x, xmax), xmin)
