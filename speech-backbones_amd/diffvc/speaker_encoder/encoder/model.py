"""SpeakerEncoder -- the module tree of DiffVC/speaker_encoder/encoder/model.py:14-63 (attribute names and therefore state_dict keys:
`lstm.*`, `linear.*`, `similarity_weight`, `similarity_bias`), so a reference checkpoint's `model_state` loads strictly.

forward() on a float32 HIP tensor with no initial state and autograd off is the kernel path of csrc/spk.hip (gtts_spk_forward: per layer
one input-projection launch and one persistent recurrence launch, then the head).  Anything else -- CPU tensors, autograd on, a given
initial state, another dtype -- runs the same modules in torch.  The GE2E training methods are out of scope and say so."""
import torch
from torch import nn

from .params_data import mel_n_channels
from .params_model import model_embedding_size, model_hidden_size, model_num_layers


def _backend():
    import importlib.util
    import os
    import sys
    try:
        from .... import _lib
        return _lib
    except (ImportError, ValueError):       # imported as the top-level package `encoder` (sys.path.append('speaker_encoder/'))
        name = "gradtts_mi355x_lib"
        if name not in sys.modules:
            here = os.path.dirname(os.path.abspath(__file__))
            path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(here))), "_lib.py")
            spec = importlib.util.spec_from_file_location(name, path)
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
        return sys.modules[name]


_TRAINING = ("SpeakerEncoder.%s belongs to GE2E training (similarity matrix, loss, EER; the reference needs sklearn, scipy and "
             "numpy's removed np.int for it), which this package does not provide: it covers inference only")


class SpeakerEncoder(nn.Module):
    def __init__(self, device, loss_device):
        super().__init__()
        self.loss_device = loss_device
        self.lstm = nn.LSTM(input_size=mel_n_channels, hidden_size=model_hidden_size, num_layers=model_num_layers,
                            batch_first=True).to(device)
        self.linear = nn.Linear(in_features=model_hidden_size, out_features=model_embedding_size).to(device)
        self.relu = nn.ReLU().to(device)
        # GE2E cosine-similarity scale and offset: part of every checkpoint, unused at inference
        self.similarity_weight = nn.Parameter(torch.tensor([10.], device=loss_device))
        self.similarity_bias = nn.Parameter(torch.tensor([-5.], device=loss_device))
        self._hip = None            # SpkPlan (host metadata)
        self._hip_packed = {}       # str(device) -> (key, flat copy of the parameters, packed blob)

    # ---- kernel path
    def invalidate_packed(self):
        self._hip_packed = {}

    def _kernel_ok(self, x, hidden_init):
        return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and hidden_init is None
                and not torch.is_grad_enabled() and self.linear.weight.device == x.device)

    def _packed(self, device):
        """The plan and the packed weights for `device`, packed again when a parameter was replaced, moved or written (address and
        version counter) -- and when its VALUE differs from the copy kept at pack time, which also catches writes through `p.data`
        that bump no version: one concatenation and one comparison on the device per call."""
        if self._hip is None:
            self._hip = _backend().SpkPlan(mel_n_channels, model_hidden_size, model_num_layers, model_embedding_size)
        state = dict(self.named_parameters())
        params = [state[name] for name, _ in self._hip.param_layout()]
        key = tuple((p.data_ptr(), p._version) for p in params)
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        ent = self._hip_packed.get(str(device))
        if ent is None or ent[0] != key or not torch.equal(ent[1], flat):
            ent = (key, flat, self._hip.pack(state, device))
            self._hip_packed[str(device)] = ent
        return self._hip, ent[2]

    def forward(self, utterances, hidden_init=None):
        """utterances [batch, n_frames, mel_n_channels] -> L2-normalised embeddings [batch, model_embedding_size]."""
        if self._kernel_ok(utterances, hidden_init):
            plan, blob = self._packed(utterances.device)
            return plan.forward(blob, utterances)
        out, (hidden, cell) = self.lstm(utterances, hidden_init)
        embeds_raw = self.relu(self.linear(hidden[-1]))
        return embeds_raw / torch.norm(embeds_raw, dim=1, keepdim=True)

    def forward_partials(self, frames, n_partials, frame_step, n_frames):
        """frames [U, T_total, mel_n_channels]: the embeddings of the partial utterances frames[u, p * frame_step : p * frame_step +
        n_frames], p < n_partials, as [U * n_partials, E], and per utterance their mean, renormalised, as [U, E] (inference.py:140-151
        of the reference).  On the kernel path the slicing is load addressing: no loop over partials, no stacked copy."""
        if self._kernel_ok(frames, None):
            plan, blob = self._packed(frames.device)
            return plan.forward(blob, frames, P=n_partials, S=frame_step, T=n_frames, want_utt=True)
        U = frames.shape[0]
        stacked = torch.stack([frames[u, p * frame_step:p * frame_step + n_frames] for u in range(U) for p in range(n_partials)], 0)
        partial = self.forward(stacked)
        raw = partial.view(U, n_partials, -1).mean(dim=1)
        return partial, raw / torch.linalg.norm(raw, dim=-1, keepdim=True)

    # ---- GE2E training: out of scope
    def do_gradient_ops(self):
        raise NotImplementedError(_TRAINING % "do_gradient_ops")

    def similarity_matrix(self, embeds):
        raise NotImplementedError(_TRAINING % "similarity_matrix")

    def loss(self, embeds):
        raise NotImplementedError(_TRAINING % "loss")
