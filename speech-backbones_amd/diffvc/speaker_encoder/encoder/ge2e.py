"""SpeakerEncoder with GE2E training -- what DiffVC/speaker_encoder/encoder/train.py needs of model.py:14-137: forward with autograd,
similarity_matrix, loss and do_gradient_ops.  `from encoder.ge2e import SpeakerEncoder` in place of `from encoder.model import
SpeakerEncoder` is the one line a copy of the reference's train.py changes; constructor, attribute names and state_dict keys are the
inference class's (encoder/model.py, which stays inference-only), so checkpoints move freely between the two.

forward() on a float32 HIP tensor with autograd on and no initial state is a torch.autograd.Function over csrc/spk_train.hip: its forward
is the inference forward keeping gates, cell states and hidden sequences (SpkPlan.forward_train; the embeddings are the inference
path's, bit for bit), its backward one persistent recurrence launch per layer plus dense products (SpkPlan.backward).  The parameters
are inputs of the Function, so .grad lands on them; the frames get no gradient.  Anything else is the parent's behaviour.

similarity_matrix() and loss() on float32 HIP embeddings run the GE2E kernel: similarity matrix, loss and the gradients for embeddings,
similarity_weight and similarity_bias in one launch (the matrix returned by the kernel path carries no gradient of its own: differentiate
through loss()).  On the CPU, or in another dtype, they are a vectorised torch restatement -- no Python loop over speakers, no np.int.
The EER is the reference's recipe on the host (sklearn, scipy: imported when it is asked for); loss(embeds, want_eer=False) skips it and
its device-to-host copy and returns (loss, None)."""
import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_

from .model import SpeakerEncoder as _InferenceEncoder
from .model import _backend


class _EncoderFn(torch.autograd.Function):
    """embeds = encoder(frames; parameters in SpkPlan.param_layout() order)."""

    @staticmethod
    def forward(ctx, module, frames, *params):
        plan, blob, blob_train = module._packed_train(frames.device)
        frames = frames.detach().contiguous()
        embeds, saved = plan.forward_train(blob, frames)
        ctx.plan, ctx.blob_train, ctx.frames, ctx.saved = plan, blob_train, frames, saved
        return embeds

    @staticmethod
    def backward(ctx, d_embeds):
        if ctx.saved is None:
            raise RuntimeError("the speaker encoder's saved state was consumed by an earlier backward (the kernels write the gate "
                               "gradients over the gates): run the forward again")
        grads = ctx.plan.backward(ctx.blob_train, ctx.frames, d_embeds, ctx.saved)
        ctx.saved = None
        return (None, None) + tuple(grads)


class _Ge2eFn(torch.autograd.Function):
    """(sim [S U, S], loss [1]) = GE2E(embeds [S, U, E], w, b); the gradient flows through loss alone."""

    @staticmethod
    def forward(ctx, embeds, w, b):
        want = any(ctx.needs_input_grad)
        sim, loss, d_embeds, dw, db = _backend().ge2e_loss(embeds.detach(), w.detach(), b.detach(), want_grad=want)
        ctx.grads = (d_embeds, dw, db)
        ctx.mark_non_differentiable(sim)
        return sim, loss

    @staticmethod
    def backward(ctx, _d_sim, d_loss):
        d_embeds, dw, db = ctx.grads
        return d_embeds * d_loss, dw * d_loss, db * d_loss


def similarity_torch(embeds, weight, bias):
    """model.py:65-107 of the reference without its loop: [S, U, E] -> [S, U, S]."""
    S, U = embeds.shape[:2]
    incl = torch.mean(embeds, dim=1, keepdim=True)
    incl = incl / torch.norm(incl, dim=2, keepdim=True)
    excl = (torch.sum(embeds, dim=1, keepdim=True) - embeds) / (U - 1)
    excl = excl / torch.norm(excl, dim=2, keepdim=True)
    sim = (embeds[:, :, None, :] * incl[None, None, :, 0, :]).sum(dim=3)        # the reference's products and sums, all j at once
    own = (embeds * excl).sum(dim=2)
    eye = torch.eye(S, dtype=torch.bool, device=embeds.device)[:, None, :]
    sim = torch.where(eye, own[:, :, None], sim)
    return sim * weight + bias


def equal_error_rate(sim, utterances_per_speaker):
    """model.py:128-135 of the reference: sim [S U, S] (numpy) with rows ordered by speaker -> EER."""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn.metrics import roc_curve
    S = sim.shape[1]
    labels = np.repeat(np.eye(S, dtype=np.int64), utterances_per_speaker, axis=0)
    fpr, tpr, _ = roc_curve(labels.flatten(), np.asarray(sim).flatten())
    return brentq(lambda x: 1. - x - interp1d(fpr, tpr)(x), 0., 1.)


class SpeakerEncoder(_InferenceEncoder):
    def __init__(self, device, loss_device):
        super().__init__(device, loss_device)
        self._hip_packed_train = {}      # str(device) -> (the inference blob it was packed beside, training blob)

    def invalidate_packed(self):
        super().invalidate_packed()
        self._hip_packed_train = {}

    def _packed_train(self, device):
        """_packed() of the parent plus the training blob, packed again whenever the inference blob was."""
        plan, blob = self._packed(device)
        ent = self._hip_packed_train.get(str(device))
        if ent is None or ent[0] is not blob:
            ent = (blob, plan.pack_train(dict(self.named_parameters()), device))
            self._hip_packed_train[str(device)] = ent
        return plan, blob, ent[1]

    def _train_kernel_ok(self, x, hidden_init):
        return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and hidden_init is None
                and torch.is_grad_enabled() and self.linear.weight.device == x.device and self.lstm.weight_hh_l0.device == x.device)

    def forward(self, utterances, hidden_init=None):
        if self._train_kernel_ok(utterances, hidden_init):
            if self._hip is None:
                self._hip = _backend().SpkPlan(self.lstm.input_size, self.lstm.hidden_size, self.lstm.num_layers, self.linear.out_features)
            state = dict(self.named_parameters())
            return _EncoderFn.apply(self, utterances, *[state[name] for name, _ in self._hip.param_layout()])
        return super().forward(utterances, hidden_init)

    # ---- GE2E
    def _ge2e_kernel_ok(self, embeds):
        return (embeds.is_cuda and embeds.dtype == torch.float32 and embeds.dim() == 3
                and self.similarity_weight.device == embeds.device and self.similarity_bias.device == embeds.device
                and self.similarity_weight.dtype == torch.float32)

    def do_gradient_ops(self):
        self.similarity_weight.grad *= 0.01
        self.similarity_bias.grad *= 0.01
        clip_grad_norm_(self.parameters(), 3, norm_type=2)

    def similarity_matrix(self, embeds):
        """embeds [speakers, utterances, embed] -> [speakers, utterances, speakers]."""
        S, U = embeds.shape[:2]
        if self._ge2e_kernel_ok(embeds):
            with torch.no_grad():
                return _Ge2eFn.apply(embeds, self.similarity_weight, self.similarity_bias)[0].view(S, U, S)
        return similarity_torch(embeds, self.similarity_weight, self.similarity_bias)

    def loss(self, embeds, want_eer=True):
        """-> (loss, EER of the batch); want_eer=False: (loss, None) without the host round trip."""
        S, U = embeds.shape[:2]
        if self._ge2e_kernel_ok(embeds):
            sim, loss = _Ge2eFn.apply(embeds, self.similarity_weight, self.similarity_bias)
            loss = loss.reshape(())
        else:
            sim = self.similarity_matrix(embeds).reshape(S * U, S)
            target = torch.arange(S, device=sim.device).repeat_interleave(U)
            loss = torch.nn.functional.cross_entropy(sim, target)
        if not want_eer:
            return loss, None
        return loss, equal_error_rate(sim.detach().cpu().numpy(), U)
