"""1:N identification: the k best-scoring entries of an enrolled gallery for every probe (csrc/nplda_topk.hip).

The reference scores listed trials only.  Here a gallery of x-vectors is embedded ONCE (utils/models.py:366-370 per entry),
and every search embeds its probes and runs ops.topk_scores against the resident embedding table: the probes x gallery score
matrix (utils/models.py:372-376 on every pair) is never written.  design/k19_topk_search.md has the semantics.
"""
import torch

from . import ops
from .adaptive_score_normalization import _model_params


def embed_table(model, x, packed):
    """(z (N, packed.ldz) with zero pad columns, q (N,)) of the model's own extract_plda_embeddings(x) on the image's
    device: the operands ops.topk_scores / ops.cohort_stats take.  q_i = sum_d Q_d z_id^2 is half the score of (z_i, z_i)
    under P = 0 (Q (z^2 + z^2); the halving is exact), so the scoring kernel gives it from the table alone."""
    dev = packed.device
    with torch.no_grad():
        z = model.extract_plda_embeddings(x)
        z = z.detach().to(device=dev, dtype=torch.float32)
        zt = torch.zeros((z.shape[0], packed.ldz), dtype=torch.float32, device=dev)
        zt[:, :packed.D2] = z
        prm = _model_params(model, dev)
        zv = zt[:, :packed.D2]
        q = ops.score_embeddings(zv, zv, torch.zeros_like(prm[4]), prm[5]).mul_(0.5)
    return zt, q


def _search_device(model, x):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    p = model.P_sqrt
    if p.is_cuda:
        return p.device
    from .models import _compute_device
    return _compute_device()


def model_stamp(model):
    """(storage address, autograd version) of every parameter and buffer of the model: the head's six tensors and, for
    Etdnn_Xvec_NeuralPlda, the extractor's weights and batch-norm statistics — all that extract_plda_embeddings reads."""
    return tuple((t.data_ptr(), t._version) for t in list(model.parameters()) + list(model.buffers()))


class Gallery:
    """An enrolled set made ready once per (model, gallery): the parameter image and the gallery's embeddings z, q, with the
    entries' ids, labels (for `exclude_labels`) and groups (for `probe_groups`) if given.  Valid while the model's parameters
    and buffers (an extractor's included) are unchanged: `check(model)`, which `search` calls, raises once they are not."""

    def __init__(self, model, packed, z, q, ids=None, labels=None, groups=None, stamp=None):
        self.model, self.packed, self.z, self.q = model, packed, z, q
        self.ids = None if ids is None else list(ids)
        self.labels, self.groups, self.stamp = labels, groups, stamp
        if self.ids is not None and len(self.ids) != z.shape[0]:
            raise ValueError("one id per gallery entry")

    def __len__(self):
        return self.z.shape[0]

    @classmethod
    def build(cls, model, x_gallery, ids=None, labels=None, groups=None):
        if not hasattr(model, "P_sqrt") or not hasattr(model, "centering_and_wccn_plda"):
            raise NotImplementedError("a Gallery searches with the NeuralPlda score (P_sqrt, Q); this model has another head")
        dev = _search_device(model, x_gallery)
        with torch.no_grad():
            packed = ops.pack_params(*_model_params(model, dev))
        z, q = embed_table(model, x_gallery, packed)
        M = z.shape[0]
        labels = None if labels is None else ops._labels(labels, "labels", M, dev)
        groups = None if groups is None else ops._labels(groups, "groups", M, dev)
        return cls(model, packed, z, q, ids, labels, groups, model_stamp(model))

    def check(self, model=None):
        """Raise if the model's parameters were modified or replaced since build(): the embeddings are the OLD model's."""
        model = self.model if model is None else model
        if self.stamp is not None and model_stamp(model) != self.stamp:
            raise ValueError("the model's parameters changed since this Gallery was built: build it again")

    def search(self, x_probe, k=10, largest=True, exclude_labels=None, probe_groups=None):
        """(scores (R, k) float32, indices (R, k) int64 into the gallery; -1 and -inf / +inf where a probe has fewer than k
        eligible entries), best first.  exclude_labels (R,): entries whose label equals the probe's are not returned;
        probe_groups (R,): a probe is searched inside its group only."""
        self.check()
        zr, qr = embed_table(self.model, x_probe, self.packed)
        labels = mask = groups = None
        if exclude_labels is not None:
            if self.labels is None:
                raise ValueError("exclude_labels needs a gallery built with labels")
            labels, mask = (exclude_labels, self.labels), "different"
        if probe_groups is not None:
            if self.groups is None:
                raise ValueError("probe_groups needs a gallery built with groups")
            groups = (probe_groups, self.groups)
        return ops.topk_scores(zr, qr, self.z, self.q, self.packed, k, largest=largest, labels=labels, mask=mask, groups=groups)

    def ids_of(self, indices):
        """Gallery ids of an index tensor from search() (any shape), None where the index is -1 -> nested lists."""
        if self.ids is None:
            raise ValueError("the gallery was built without ids")
        def walk(v):
            return [walk(e) for e in v] if isinstance(v, list) else (self.ids[v] if v >= 0 else None)
        return walk(torch.as_tensor(indices).cpu().tolist())
