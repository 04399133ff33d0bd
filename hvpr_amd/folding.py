"""Eval-mode BatchNorm folding shared by the modules: y = x*s + t with s = gamma/sqrt(var+eps), t = beta - mean*s."""
import torch
import torch.nn as nn


def bn_scale_shift(bn):
    s = bn.weight.detach() / torch.sqrt(bn.running_var.detach() + bn.eps)
    return s.float(), (bn.bias.detach() - bn.running_mean.detach() * s).float()


class FoldCache:
    """Folded weights are rebuilt when the module returns to eval mode, after load_state_dict, on device moves, or on
    an explicit invalidate(); mutating parameters by hand while in eval mode needs invalidate()."""

    def __init__(self):
        self.value = None
        self.device = None

    def invalidate(self):
        self.value = None

    def get(self, device, build):
        if self.value is None or self.device != device:
            with torch.no_grad():
                self.value = build()
            self.device = device
        return self.value


class FoldCached(nn.Module):
    """A module whose eval forward runs on folded / packed weights kept in `self._fold`: train() and load_state_dict() drop them.
    List it in front of the module's other bases.  detector._CapturedState finds these modules by this class."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._fold = FoldCache()

    def train(self, mode=True):
        self._fold.invalidate()
        return super().train(mode)

    def _load_from_state_dict(self, *a, **k):
        self._fold.invalidate()
        return super()._load_from_state_dict(*a, **k)
