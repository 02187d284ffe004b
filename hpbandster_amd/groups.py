"""Grouped KDE models: B independent brackets refit, sampled and acquired in one call each.

Config #5's loop on the device from end to end::

    gm = groups.fit_groups(X, losses, seg_off, var_type)      # hbx_seg_argsort_ex + hbx_kde_fit
    rows, picks = gm.propose(64, seed, levels)                # hbx_kde_sample_groups + hbx_kde_acquire_groups
    rows, picks = gm.propose(64, seed, levels, requests=S)    # S picks per bracket: hbx_kde_acquire_groups_batch
    rows, top = gm.propose(64, seed, levels, topk=k)          # the k best of each pool: hbx_kde_acquire_groups_topk
    lp = gm.logpdf(cands)                                     # ln l, ln g of every candidate: hbx_kde_logpdf_groups
    cfg = gm.get_config(64, seed, levels, requests=S)         # a configuration per request, prior draws where the
                                                              # reference falls back: hbx_kde_propose_groups
    opt = GroupBOHB(B, var_type, levels)                      # B BOHB runs in lockstep: new_results / get_configs
    nxt, src, counts = advance(rows, seg_off, mask, K, fresh) # the next SH stage of every bracket: hbx_sh_advance_groups
    res = GroupHyperband(opt, eta, min_b, max_b).run(n, f)    # B Hyperband runs: GroupSuccessiveHalving per iteration

Bracket b owns the rows ``X[seg_off[b]:seg_off[b+1]]``; its good / bad KDEs are the head ``n_good[b]`` / tail
``n_bad[b]`` rows of numpy's argsort of its losses (bohb.py:220-246).  The fit's outputs (order, bandwidths, level
counts) stay on the device and are read there by the sampler and the acquisition: no host round trip between the
steps.  Every pick is the reference's (bohb.py:124-169 on that bracket's pair): index, score and both pdfs bit
for bit.  The drop-in ``BOHB`` class is not involved; this is the batched engine surface.
"""

import ctypes

import numpy as np

from . import _native as N
from . import kde

ACQ_NO_MODEL, ACQ_UNSUPPORTED = 16, 32  # include/hbx.h HBX_ACQ_*

# one result record (include/hbx.h hbx_kde_result_ptr), 48 bytes
RECORD = np.dtype([("index", "<i8"), ("score", "<f8"), ("rel", "<f4"), ("flags", "<i4"), ("shortlist", "<i4"),
                   ("near", "<i4"), ("pdf_l", "<f8"), ("pdf_g", "<f8")])
assert RECORD.itemsize == kde.RESULT_BYTES


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _to_device(a, dtype, device, strict=False, what=None):
    """Host array or tensor ``a`` as a contiguous device tensor of ``dtype``.  Lenient: a tensor is converted, moved
    and made contiguous where it is not.  ``strict``: a tensor is used where it lies and must be contiguous and of
    ``dtype`` already (bool counts as uint8) -- HbxError naming ``what`` otherwise."""
    torch = kde._torch()
    if not _is_tensor(a):
        npd = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, dtype=npd)).to(device)
    if not strict:
        return a.to(device=device, dtype=dtype).contiguous()
    t = a.view(torch.uint8) if a.dtype == torch.bool and dtype == torch.uint8 else a
    if t.dtype != dtype or not t.is_contiguous():
        raise N.HbxError("%s must be a contiguous %s tensor" % (what, dtype))
    return t


def _philox(seed, counter_base, stream_id):
    """(seed, counter_base, stream_id) as the calls take them: u64, u64, u32"""
    return int(seed) & (2 ** 64 - 1), int(counter_base) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF


def _gather_rows(cands, group_index, candidate_index):
    """``cands[group_index, candidate_index]`` on the host: ``cands`` [G, C, D], numpy or a device tensor (only the
    indexed rows are fetched); the indices are host int64 arrays."""
    if _is_tensor(cands):
        torch = kde._torch()
        return cands[torch.from_numpy(group_index).to(cands.device),
                     torch.from_numpy(candidate_index).to(cands.device)].cpu().numpy()
    return np.asarray(cands, dtype=np.float64)[group_index, candidate_index]


class GroupPicks(object):
    """One pick per group (hbx_kde_acquire_groups), from one fetch of the B records: numpy arrays ``index``
    (int64, relative to the group's pool, -1: no pick), ``score``, ``pdf_l``, ``pdf_g`` (float64, the reference's
    values bit for bit), ``rel`` (float32), ``flags`` (kde.ACQ_* and ACQ_NO_MODEL / ACQ_UNSUPPORTED), ``shortlist``
    and ``near`` (int32), each of length B -- or, one pick per request (hbx_kde_acquire_groups_batch), of shape
    [B, S] with ``index`` relative to the request's own pool.  ``len()`` is B either way."""
    __slots__ = ("index", "score", "pdf_l", "pdf_g", "rel", "flags", "shortlist", "near")

    def __init__(self, records):
        r = np.asarray(records, dtype=RECORD)
        for name in self.__slots__:
            setattr(self, name, np.ascontiguousarray(r[name]))

    @classmethod
    def from_bytes(cls, b, B, S=None):
        """B records (``S`` None), or B * S records in request order b * S + s, as arrays of shape [B, S]."""
        if S is None:
            return cls(np.frombuffer(bytes(b), dtype=RECORD, count=B))
        return cls(np.frombuffer(bytes(b), dtype=RECORD, count=B * S).reshape(B, S))

    def __len__(self):
        return int(self.index.shape[0])

    def rows(self, cands):
        """The winning candidate rows on the host, float64; NaN rows where ``index < 0``.  ``cands`` (numpy or a
        device tensor): [B, C, D] gives [B, D]; [B, S, C, D], with picks of shape [B, S], gives [B, S, D]."""
        lead = tuple(int(v) for v in cands.shape[:-2])
        if lead != self.index.shape:
            raise N.HbxError("candidates %s do not match picks %s" % (tuple(cands.shape), self.index.shape))
        C, D = int(cands.shape[-2]), int(cands.shape[-1])
        index = self.index.reshape(-1)
        out = np.full((index.size, D), np.nan)
        ok = np.nonzero(index >= 0)[0]
        if ok.size:
            out[ok] = _gather_rows(cands.reshape(-1, C, D), ok, index[ok])
        return out.reshape(lead + (D,))

    def __repr__(self):
        if self.index.ndim == 2:
            return "GroupPicks(B=%d, S=%d, picked=%d)" % (self.index.shape + (int((self.index >= 0).sum()),))
        return "GroupPicks(B=%d, picked=%d)" % (len(self), int((self.index >= 0).sum()))


class GroupTopK(object):
    """The k best candidates of every group's pool (hbx_kde_acquire_groups_topk), ranked by (score, index), from one
    fetch of the B result blocks: ``count``, ``shortlist``, ``flags`` (int32 [B]; kde.ACQ_* and ACQ_NO_MODEL /
    ACQ_UNSUPPORTED); ``index`` (int64 [B, k], relative to the group's pool, -1 past ``count``); ``score``,
    ``pdf_l``, ``pdf_g`` (float64 [B, k], the reference's values bit for bit, NaN past ``count``); ``rel`` (float32
    [B, k], 0 past ``count``).  ``len()`` is B."""
    __slots__ = ("k", "count", "shortlist", "flags", "index", "score", "pdf_l", "pdf_g", "rel")

    def __init__(self, B, k):
        self.k = int(k)
        self.count = np.zeros(B, dtype=np.int32)
        self.shortlist = np.zeros(B, dtype=np.int32)
        self.flags = np.zeros(B, dtype=np.int32)
        self.index = np.full((B, self.k), -1, dtype=np.int64)
        self.score = np.full((B, self.k), np.nan)
        self.pdf_l = np.full((B, self.k), np.nan)
        self.pdf_g = np.full((B, self.k), np.nan)
        self.rel = np.zeros((B, self.k), dtype=np.float32)

    @classmethod
    def from_bytes(cls, b, B, k):
        """B blocks of 16 + 40 k bytes (include/hbx.h hbx_kde_acquire_groups_topk); the bytes of a block past its
        ``count`` records are not read."""
        B, k = int(B), int(k)
        step = kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * k
        raw = np.frombuffer(bytes(b), dtype=np.uint8, count=B * step).reshape(B, step)
        out = cls(B, k)
        head = np.ascontiguousarray(raw[:, :kde.TOPK_HEAD_BYTES]).view("<i4").reshape(B, 4)
        out.count[:], out.shortlist[:], out.flags[:] = head[:, 0], head[:, 1], head[:, 2]
        if np.any(out.count < 0) or np.any(out.count > k):
            raise N.HbxError("top-k blocks: a count outside [0, %d]" % k)
        rec = np.ascontiguousarray(raw[:, kde.TOPK_HEAD_BYTES:]).view(kde.TOPK_REC).reshape(B, k)
        live = np.arange(k)[None, :] < out.count[:, None]
        for name in ("index", "score", "pdf_l", "pdf_g", "rel"):
            getattr(out, name)[live] = rec[name][live]
        return out

    def __len__(self):
        return int(self.count.shape[0])

    def top(self, b):
        """Group b's entries as a kde.TopK."""
        c = int(self.count[b])
        return kde.TopK(self.index[b, :c].copy(), self.score[b, :c].copy(), self.pdf_l[b, :c].copy(),
                        self.pdf_g[b, :c].copy(), self.rel[b, :c].copy(), int(self.shortlist[b]), int(self.flags[b]))

    def rows(self, cands):
        """The ranked candidate rows on the host, float64 [B, k, D]; NaN rows past ``count``.  ``cands``: [B, C, D],
        numpy or a device tensor."""
        if len(cands.shape) != 3 or int(cands.shape[0]) != len(self):
            raise N.HbxError("candidates %s do not match %d groups" % (tuple(cands.shape), len(self)))
        D = int(cands.shape[2])
        out = np.full((len(self), self.k, D), np.nan)
        bi, ji = np.nonzero(self.index >= 0)
        if bi.size:
            out[bi, ji] = _gather_rows(cands, bi, self.index[bi, ji])
        return out

    def __repr__(self):
        return "GroupTopK(B=%d, k=%d, returned=%d)" % (len(self), self.k, int(self.count.sum()))


SOURCE_MODEL, SOURCE_RANDOM_FRACTION, SOURCE_NO_MODEL, SOURCE_NO_SCORE, SOURCE_DOMAIN_ERR = 0, 1, 2, 3, 4  # HBX_CFG_*
SOURCE_SKIPPED = 5           # HBX_CFG_SKIPPED: the request mask left the request out (its row is NaN)
ACQ_SKIPPED = 64             # include/hbx.h HBX_ACQ_SKIPPED: the record of such a request
PROPOSE_SKIP_RANDOM = 1      # include/hbx.h HBX_PROPOSE_SKIP_RANDOM


def counts_to_mask(counts, S):
    """The request mask of per-run request counts: ``counts`` [B] (an int array, or an int device tensor) ->
    uint8 [B, S] with request (b, s) wanted iff ``s < counts[b]``; a tensor op where ``counts`` lies, no read-back."""
    S = int(S)
    if _is_tensor(counts):
        torch = kde._torch()
        if counts.dim() != 1 or counts.dtype not in (torch.int64, torch.int32):
            raise N.HbxError("counts must be an int32 / int64 tensor [B], got %s %s" % (counts.dtype,
                                                                                      tuple(counts.shape)))
        return (torch.arange(S, device=counts.device)[None, :] < counts[:, None]).to(torch.uint8)
    c = np.asarray(counts)
    if c.ndim != 1 or c.dtype.kind not in "iu":
        raise N.HbxError("counts must be an int array [B], got %s %s" % (c.dtype, c.shape))
    return (np.arange(S)[None, :] < c[:, None]).astype(np.uint8)


def request_mask(want, B, S, device):
    """``want`` as the contiguous uint8 device tensor [B, S] the masked calls read (None stays None: every request).
    ``want``: a bool / uint8 array or contiguous device tensor [B, S], or per-run counts -- an int array or device
    tensor [B] (counts_to_mask).  HbxError for another dtype, shape, device or memory order, before any launch."""
    if want is None:
        return None
    torch = kde._torch()
    B, S = int(B), int(S)
    if _is_tensor(want):
        if want.device.type != torch.device(device).type or (
                torch.device(device).index is not None and want.device.index != torch.device(device).index):
            raise N.HbxError("the request mask must lie on %s, got a tensor on %s" % (device, want.device))
        if want.dim() == 1 and want.dtype in (torch.int64, torch.int32):
            if int(want.shape[0]) != B:
                raise N.HbxError("counts must have %d entries, got %d" % (B, int(want.shape[0])))
            return counts_to_mask(want, S)
        if want.dtype not in (torch.bool, torch.uint8):
            raise N.HbxError("the request mask must be bool or uint8, got %s" % (want.dtype,))
        if tuple(want.shape) != (B, S):
            raise N.HbxError("the request mask must be [%d, %d], got %s" % (B, S, tuple(want.shape)))
        if not want.is_contiguous():
            raise N.HbxError("the request mask must be contiguous")
        return want.view(torch.uint8) if want.dtype == torch.bool else want
    w = np.asarray(want)
    if w.ndim == 1 and w.dtype.kind in "iu" and w.dtype != np.uint8:
        if w.shape[0] != B:
            raise N.HbxError("counts must have %d entries, got %d" % (B, w.shape[0]))
        w = counts_to_mask(w, S)
    if w.dtype not in (np.bool_, np.uint8):
        raise N.HbxError("the request mask must be bool or uint8, got %s" % (w.dtype,))
    if w.shape != (B, S):
        raise N.HbxError("the request mask must be [%d, %d], got %s" % (B, S, w.shape))
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.uint8)).to(device)


class GroupConfigs(object):
    """One configuration vector per get_config request (hbx_kde_finish_groups / hbx_kde_propose_groups): ``rows``
    (float64 [B, S, D], or [B, D] when the call had no ``requests``), ``source`` (uint8 [B, S] or [B]: SOURCE_MODEL
    the winning candidate's row, anything else a prior draw and why -- bohb.py:107-111,154-166), ``model_based``
    (``source == SOURCE_MODEL``: the reference's info_dict['model_based_pick']) and ``picks`` (the acquisition's
    records, None when they were not requested).  Host arrays and a GroupPicks after a synchronising call; with
    ``sync=False`` device tensors, ``picks`` the device tensor of the records (uint8 [B, S, 48] or [B, 48]).
    ``cands`` / ``domain_err`` hold the pools and the sampler's error bytes when the call kept them.  ``len()`` is B."""
    SOURCE_MODEL, SOURCE_RANDOM_FRACTION, SOURCE_NO_MODEL, SOURCE_NO_SCORE, SOURCE_DOMAIN_ERR = \
        SOURCE_MODEL, SOURCE_RANDOM_FRACTION, SOURCE_NO_MODEL, SOURCE_NO_SCORE, SOURCE_DOMAIN_ERR  # (the module's)
    SOURCE_SKIPPED = SOURCE_SKIPPED  # a request the mask left out: a NaN row, not model based
    __slots__ = ("rows", "source", "model_based", "picks", "cands", "domain_err")

    def __init__(self, rows, source, B, S=None, picks=None, cands=None, domain_err=None):
        lead = (int(B),) if S is None else (int(B), int(S))
        self.rows = rows.reshape(lead + (int(rows.shape[-1]),))
        self.source = source.reshape(lead)
        self.model_based = self.source == self.SOURCE_MODEL
        self.picks, self.cands, self.domain_err = picks, cands, domain_err

    def __len__(self):
        return int(self.source.shape[0])

    def __repr__(self):
        return "GroupConfigs(shape=%s)" % (tuple(self.source.shape),)


def _levels_dev(levels, D, device):
    """``levels`` (D level counts, 0: continuous) as an int32 device tensor; a tensor already there is used as is."""
    torch = kde._torch()
    if _is_tensor(levels):
        if levels.dtype != torch.int32 or tuple(levels.shape) != (D,) or not levels.is_contiguous():
            raise N.HbxError("levels tensor must be contiguous int32 [%d]" % D)
        return levels.to(device)
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32))
    if lv.shape != (D,):
        raise N.HbxError("levels must have %d entries" % D)
    return torch.from_numpy(lv).to(device)


def _fraction(random_fraction):
    rf = float(random_fraction)
    if not 0.0 <= rf <= 1.0:
        raise ValueError("random_fraction must be in [0, 1], got %r" % (random_fraction,))
    return rf


def _configs(rows, source, B, S, sync, records=None, cands=None, err=None):
    """GroupConfigs from the device outputs of one call (inside its on_device context)"""
    if not sync:
        if records is not None:
            records = records.view((B, kde.RESULT_BYTES) if S is None else (B, S, kde.RESULT_BYTES))
        return GroupConfigs(rows, source, B, S, records, cands, err)
    picks = None if records is None else GroupPicks.from_bytes(records.cpu().numpy().tobytes(), B, S)
    return GroupConfigs(rows.cpu().numpy(), source.cpu().numpy(), B, S, picks,
                        None if cands is None else cands.cpu().numpy(), None if err is None else err.cpu().numpy())


def _finish(device, stream, B, S, C, D, records, cands, err, levels, random_fraction, seed, counter_base, stream_id,
            want=None):
    """one hbx_kde_finish_groups launch over device tensors (records None: NULL); (rows [B * S, D], source [B * S]).
    ``want``: the request mask (request_mask's tensor) -- then hbx_kde_finish_groups_m."""
    torch = kde._torch()
    Sn = 1 if S is None else int(S)
    rows = torch.empty((B * Sn, D), dtype=torch.float64, device=device)
    source = torch.empty(B * Sn, dtype=torch.uint8, device=device)
    lvd = _levels_dev(levels, D, device)
    head = (N.ptr(records), N.ptr(cands), N.ptr(err), N.ptr(lvd), D, B, Sn, int(C), random_fraction) + \
        _philox(seed, counter_base, stream_id)
    tail = (N.ptr(rows), N.ptr(source), N.stream_handle(stream, device))
    if want is None:
        N.check(N.lib().hbx_kde_finish_groups(*(head + tail)))
    else:
        N.check(N.lib().hbx_kde_finish_groups_m(*(head + (N.ptr(want),) + tail)))
    return rows, source


def sample_prior(B, S, levels, seed, counter_base=0, C=1, stream=None, stream_id=0, device=None, sync=True,
                 want=None):
    """What B runs without any model answer S get_config requests each with (bohb.py:109-110): one prior draw per
    request (hbx_kde_finish_groups without records), request (b, s) on the Philox counter
    ``counter_base + (b * S + s) * C`` -- ``C`` is the counter stride, the pool size the same requests would use
    with a model.  ``S`` None: one request per run, rows [B, D].  Returns GroupConfigs, every source
    SOURCE_NO_MODEL -- or, under a request mask ``want`` (request_mask's forms), SOURCE_SKIPPED and a NaN row for the
    requests it leaves out."""
    D = len(levels) if not _is_tensor(levels) else int(levels.shape[0])
    if device is None:
        device = levels.device if _is_tensor(levels) else kde.default_device()
    with N.on_device(device, stream):
        wd = request_mask(want, B, 1 if S is None else S, device)
        rows, source = _finish(device, stream, int(B), S, C, D, None, None, None, levels, 0.0, seed, counter_base,
                               stream_id, wd)
        return _configs(rows, source, int(B), S, sync)


GRP_EXACT_L, GRP_EXACT_G = 64, 128  # include/hbx.h HBX_GRP_EXACT_*
LOGPDF_FP64_ONLY = 1                 # include/hbx.h HBX_LOGPDF_FP64_ONLY


class GroupLogPdf(object):
    """Both KDEs' log densities at every candidate of every group's pool (hbx_kde_logpdf_groups): ``ln_l`` and
    ``ln_g`` (float64, shaped like the pool's leading dims -- [B, C] or [B, S, C] --, None when not requested; -inf
    where the pdf is 0, NaN where the reference's is NaN or negative and for groups without a usable model),
    ``status`` (int32 [B]: ACQ_NO_MODEL / ACQ_UNSUPPORTED, GRP_EXACT_L / GRP_EXACT_G) and ``stats`` (4 ints: values
    written by the fp32 pass, the fp64 log-space pass, through the exact pdf, NaN-filled; None before a
    synchronisation).  With ``sync=False`` the arrays are device tensors.  ``len()`` is B."""
    __slots__ = ("ln_l", "ln_g", "status", "stats")

    def __init__(self, ln_l, ln_g, status, stats=None, lead=None):
        if lead is not None:
            ln_l = None if ln_l is None else ln_l.reshape(lead)
            ln_g = None if ln_g is None else ln_g.reshape(lead)
        self.ln_l, self.ln_g, self.status = ln_l, ln_g, status
        self.stats = None if stats is None else tuple(int(v) for v in stats)

    def __len__(self):
        return int(self.status.shape[0])

    def __repr__(self):
        shape = tuple((self.ln_l if self.ln_l is not None else self.ln_g).shape)
        return "GroupLogPdf(shape=%s, stats=%s)" % (shape, self.stats)


# include/hbx.h's names for the model parameters of the grouped entry points, in its order (hbx_kde_acquire_groups),
# and for those of the sampler, which reads the good side alone (hbx_kde_sample_groups)
MODEL_ARGS = ("X", "D", "seg_off", "B", "order", "n_good", "n_bad", "vartype", "bw_good", "bw_bad", "nlev_good",
              "nlev_bad")
SAMPLE_ARGS = ("X", "D", "seg_off", "B", "order", "n_good", "bw_good")


class GroupModel(object):
    """The KDE pairs of B brackets after one batched refit (fit_groups).  ``B``, ``D``, ``n_good`` / ``n_bad``
    (host int64[B], 0 where the reference builds no model) and ``has_model`` (host bool[B]) are host-side facts
    known before the fit; everything the fit computed stays in device tensors (``order``, ``bw_good``, ``bw_bad``,
    ``nlev_good``, ``nlev_bad``)."""

    def __init__(self, **kw):
        self.pdf_floor, self.min_bandwidth = N.PDF_FLOOR_DEFAULT, 0.0  # the rules it was fitted under (fit_groups)
        self.__dict__.update(kw)
        self._host = None
        # the hbx_rules block of the rules-taking calls; None under the reference snapshot's floor, where the
        # calls are the ones without it
        self._rules = None if self.pdf_floor == N.PDF_FLOOR_DEFAULT else N.rules(self.pdf_floor, self.min_bandwidth)

    def _call(self, name, *args):
        """Entry point ``name``, or under another score floor its rules-taking form with the model's rules."""
        if self._rules is None:
            N.check(getattr(N.lib(), name)(*args))
        else:
            N.check(getattr(N.lib(), name + "_r")(*(args + (ctypes.addressof(self._rules),))))

    def model_args(self, names=MODEL_ARGS):
        """The model arguments every grouped entry point takes first, in include/hbx.h's order (MODEL_ARGS)."""
        arg = dict(X=N.ptr(self.X), D=self.D, seg_off=N.ptr(self.seg_off), B=self.B, order=N.ptr(self.order),
                   n_good=N.ptr(self.n_good_dev), n_bad=N.ptr(self.n_bad_dev), vartype=N.ptr(self.vt_dev),
                   bw_good=N.ptr(self.bw_good), bw_bad=N.ptr(self.bw_bad), nlev_good=N.ptr(self.nlev_good),
                   nlev_bad=N.ptr(self.nlev_bad))
        return tuple(arg[name] for name in names)

    # ---- host views (checks and debugging) --------------------------------------------------------------
    def bandwidths(self):
        """(bw_good, bw_bad): host float64 [B, D] (NaN rows for groups without a model)."""
        return self.bw_good.cpu().numpy(), self.bw_bad.cpu().numpy()

    def _host_state(self):
        if self._host is None:
            self._host = dict(X=self.X.cpu().numpy(), order=self.order.cpu().numpy(),
                              bw=self.bandwidths(), nlev=(self.nlev_good.cpu().numpy(), self.nlev_bad.cpu().numpy()))
        return self._host

    def rows_of(self, b):
        """(good_rows, bad_rows) of group b: positions local to its segment, in the split's order."""
        h = self._host_state()
        s, e = int(self.seg_host[b]), int(self.seg_host[b + 1])
        o = h["order"][s:e]
        return o[:int(self.n_good[b])], o[e - s - int(self.n_bad[b]):]

    def pair(self, b):
        """Group b's model as a KDEPair built through the single path (kde.fit_pair_from_rows: two
        hbx_kde_prepare calls) -- for checks and debugging; None where the group has no model."""
        if not self.has_model[b]:
            return None
        h = self._host_state()
        s, e = int(self.seg_host[b]), int(self.seg_host[b + 1])
        g, bd = self.rows_of(b)
        return kde.fit_pair_from_rows(h["X"][s:e], g, bd, self.var_type, h["bw"][0][b], h["bw"][1][b],
                                      h["nlev"][0][b], h["nlev"][1][b], device=self.device, pdf_floor=self.pdf_floor)

    # ---- the grouped calls ------------------------------------------------------------------------------
    def sample(self, C, seed, levels, bandwidth_factor=3, counter_base=0, stream=None, stream_id=0, requests=None,
               want=None):
        """C candidates per group around its good KDE's rows (bohb.py:133-147; hbx_kde_sample_groups):
        candidate (b, i) draws from the Philox counter ``counter_base + b * C + i``.  Returns device tensors
        (cands [B, C, D] float64, domain_err [B, C] uint8); groups without a model get NaN rows.
        With ``requests=S``: S pools of C candidates per group, (cands [B, S, C, D], domain_err [B, S, C]) -- the
        same call with pool size S * C, so candidate (b, s, i) draws from the Philox counter
        ``counter_base + (b * S + s) * C + i`` and the bytes equal ``sample(S * C, ...)``'s.
        ``want`` (with ``requests``; request_mask's forms): hbx_kde_sample_groups_m -- only the wanted requests are
        drawn, with the same bytes; the rows of the others are not written (whatever the new tensor held)."""
        if want is not None:
            if requests is None:
                raise N.HbxError("sample: a request mask needs requests=S")
            torch = kde._torch()
            S, C = int(requests), int(C)
            with N.on_device(self.device, stream):
                wd = request_mask(want, self.B, S, self.device)
                lvd = _levels_dev(levels, self.D, self.device)
                cands = torch.empty((self.B, S, C, self.D), dtype=torch.float64, device=self.device)
                err = torch.zeros((self.B, S, C), dtype=torch.uint8, device=self.device)
                N.check(N.lib().hbx_kde_sample_groups_m(
                    *(self.model_args(SAMPLE_ARGS) + (N.ptr(lvd), float(bandwidth_factor)) +
                      _philox(seed, counter_base, stream_id) +
                      (S, C, N.ptr(wd), N.ptr(cands), N.ptr(err), N.stream_handle(stream, self.device)))))
            return cands, err
        if requests is not None:
            S = int(requests)
            cands, err = self.sample(S * int(C), seed, levels, bandwidth_factor, counter_base, stream, stream_id)
            return cands.view(self.B, S, int(C), self.D), err.view(self.B, S, int(C))
        torch = kde._torch()
        C = int(C)
        with N.on_device(self.device, stream):
            lvd = _levels_dev(levels, self.D, self.device)
            cands = torch.empty((self.B, C, self.D), dtype=torch.float64, device=self.device)
            err = torch.zeros((self.B, C), dtype=torch.uint8, device=self.device)
            N.check(N.lib().hbx_kde_sample_groups(
                *(self.model_args(SAMPLE_ARGS) + (N.ptr(lvd), float(bandwidth_factor)) +
                  _philox(seed, counter_base, stream_id) +
                  (C, N.ptr(cands), N.ptr(err), N.stream_handle(stream, self.device)))))
        return cands, err

    def workspace_bytes(self, C, requests=1):
        return int(N.lib().hbx_kde_groups_batch_workspace_bytes(self.B, int(requests), int(C), self.D))

    def _stage_cands(self, cands, ranks):
        """A caller's pool as the contiguous float64 device tensor the grouped calls read (the grouped twin of
        KDEPair._stage_cands).  ``ranks``: the legal ones, 3 for [B, C, D] and 4 for [B, S, C, D]."""
        torch = kde._torch()

        def want():
            return " or ".join("[%d, %s, %d]" % (self.B, "C" if r == 3 else "S, C", self.D) for r in ranks)

        if _is_tensor(cands):
            cd = cands
            if cd.dtype != torch.float64 or not cd.is_contiguous():
                raise N.HbxError("candidate tensor must be contiguous float64 %s" % want())
        else:
            cd = torch.from_numpy(np.ascontiguousarray(cands, dtype=np.float64)).to(self.device)
        if cd.dim() not in ranks or int(cd.shape[0]) != self.B or int(cd.shape[-1]) != self.D:
            raise N.HbxError("candidates must be %s, got %s" % (want(), tuple(cd.shape)))
        return cd

    def _workspace(self, workspace, needed_bytes, what):
        """The caller's workspace, or a new one, of at least ``needed_bytes``; a negative size is the size helper's
        refusal of the call's sizes, reported in the words ``what``."""
        if needed_bytes < 0:
            raise N.HbxError(what)
        torch = kde._torch()
        ws = workspace if workspace is not None else torch.empty(needed_bytes, dtype=torch.uint8, device=self.device)
        if ws.numel() < needed_bytes:
            raise N.HbxError("workspace too small")
        return ws

    def _acquire(self, cd, S, C, stream, workspace, sync, want=None):
        """``acquire`` (``S`` None) and ``acquire_requests`` over the staged pool ``cd``, inside the caller's
        on_device context: the one-request entry point for ``S`` None under the default floor, the batched one
        otherwise; records [B, 48] or [B, S, 48]."""
        torch = kde._torch()
        Sn = 1 if S is None else S
        sizes = "B * C = %d * %d" % (self.B, C) if S is None else "B * S * C = %d * %d * %d" % (self.B, S, C)
        ws = self._workspace(workspace, self.workspace_bytes(C, Sn), sizes + " exceeds int32")
        res = torch.empty((self.B, kde.RESULT_BYTES) if S is None else (self.B, S, kde.RESULT_BYTES),
                          dtype=torch.uint8, device=self.device)
        model = self.model_args() + (N.ptr(cd),)
        tail = (N.ptr(res), N.ptr(ws), ws.numel(), N.stream_handle(stream, self.device))
        if want is not None:
            N.check(N.lib().hbx_kde_acquire_groups_batch_m(*(model + (Sn, C, N.ptr(want)) + tail + (
                None if self._rules is None else ctypes.addressof(self._rules),))))
        elif S is None and self._rules is None:
            N.check(N.lib().hbx_kde_acquire_groups(*(model + (C,) + tail)))
        else:  # (the batched call's S = 1 case is the one-request call: include/hbx.h)
            self._call("hbx_kde_acquire_groups_batch", *(model + (Sn, C) + tail))
        if not sync:
            return res
        return GroupPicks.from_bytes(res.cpu().numpy().tobytes(), self.B, S)

    def acquire(self, cands, stream=None, workspace=None, sync=True):
        """Per group the first index minimising max(f, g)/max(l, f) over its own pool ``cands[b]``, f the model's
        ``pdf_floor`` (hbx_kde_acquire_groups; under another floor than 1e-8 its S = 1 rules-taking form).
        ``cands``: [B, C, D] float64, numpy or a device tensor.  Returns GroupPicks, or with ``sync=False`` the device
        tensor of the B records (uint8 [B, 48])."""
        with N.on_device(self.device, stream):
            cd = self._stage_cands(cands, (3,))
            return self._acquire(cd, None, int(cd.shape[1]), stream, workspace, sync)

    def acquire_requests(self, cands, stream=None, workspace=None, sync=True, want=None):
        """S get_config requests per group in one call (hbx_kde_acquire_groups_batch; HB_iteration.py:136-138 issues
        a stage's requests back to back against one model): request (b, s) is ``acquire`` for group b over its own
        pool ``cands[b, s]`` and sees no other request.  ``cands``: [B, S, C, D] float64, numpy or a device tensor.
        Returns GroupPicks with arrays of shape [B, S], or with ``sync=False`` the device tensor of the records
        (uint8 [B, S, 48]).  ``want`` (request_mask's forms): hbx_kde_acquire_groups_batch_m -- the wanted requests'
        records are the same bytes, the others get the empty record with ACQ_SKIPPED and their pools are not read;
        ``request_stats(workspace)`` then says what was computed."""
        with N.on_device(self.device, stream):
            cd = self._stage_cands(cands, (4,))
            wd = request_mask(want, self.B, int(cd.shape[1]), self.device)
            return self._acquire(cd, int(cd.shape[1]), int(cd.shape[2]), stream, workspace, sync, wd)

    def request_stats(self, workspace):
        """The counters of the last masked acquisition that used ``workspace`` (``acquire_requests(want=...)``, or
        ``get_config`` with a mask or ``skip_random``): (requests answered, requests skipped, candidates the screen
        evaluated, candidates re-scored in fp64).  Synchronises the device (hbx_kde_groups_request_stats)."""
        out = np.zeros(4, dtype=np.int64)
        with N.on_device(self.device):
            N.check(N.lib().hbx_kde_groups_request_stats(N.ptr(workspace), out.ctypes.data))
        return tuple(int(v) for v in out)

    def workspace_bytes_topk(self, C, k):
        return int(N.lib().hbx_kde_groups_topk_workspace_bytes(self.B, int(C), int(k), self.D))

    def acquire_topk(self, cands, k, stream=None, workspace=None, sync=True):
        """Per group the first min(k, F) entries of the ascending order by (score, index) over the F candidates of
        its own pool ``cands[b]`` whose score is not NaN (hbx_kde_acquire_groups_topk); entry 0 is ``acquire``'s
        pick.  ``cands``: [B, C, D] float64, numpy or a device tensor; 1 <= k <= kde.TOPK_MAX_K, k > C is legal.
        Returns GroupTopK, or with ``sync=False`` the device tensor of the B result blocks (uint8 [B, 16 + 40 k])."""
        torch = kde._torch()
        k = int(k)
        if k < 1 or k > kde.TOPK_MAX_K:
            raise ValueError("k must be in [1, %d], got %d" % (kde.TOPK_MAX_K, k))
        with N.on_device(self.device, stream):
            cd = self._stage_cands(cands, (3,))
            C = int(cd.shape[1])
            ws = self._workspace(workspace, self.workspace_bytes_topk(C, k),
                                 "B * C = %d * %d exceeds int32" % (self.B, C))
            res = torch.empty((self.B, kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * k), dtype=torch.uint8,
                              device=self.device)
            self._call("hbx_kde_acquire_groups_topk", *(self.model_args() + (
                N.ptr(cd), C, k, N.ptr(res), N.ptr(ws), ws.numel(), N.stream_handle(stream, self.device))))
            if not sync:
                return res
            return GroupTopK.from_bytes(res.cpu().numpy().tobytes(), self.B, k)

    def workspace_bytes_logpdf(self, C):
        return int(N.lib().hbx_kde_logpdf_groups_workspace_bytes(self.B, int(C), self.D))

    def logpdf(self, cands, rtol=1e-5, which="both", fp64_only=True, stream=None, workspace=None, sync=True):
        """ln l(x) and ln g(x) of every candidate of every group's own pool (hbx_kde_logpdf_groups): each value within
        ``rtol * max(1, |ln p|)`` of the reference's KDEMultivariate.pdf.  ``cands``: [B, C, D] or [B, S, C, D]
        float64, numpy or a contiguous device tensor; ``which``: "both", "good" (ln_l only) or "bad" (ln_g only);
        ``fp64_only=False`` runs the fp32 first pass before the fp64 one (the C ABI's flags = 0): the same contract,
        3 % faster at config #5's shape and half as fast at 8 continuous dims (DESIGN section 4 "Grouped ln-pdf"), so
        the fp64 pass alone is the default here.  Returns GroupLogPdf with host arrays, or with ``sync=False`` with
        device tensors (and ``stats`` None: reading the counters synchronises)."""
        if which not in ("both", "good", "bad"):
            raise ValueError("which must be 'both', 'good' or 'bad', got %r" % (which,))
        if not float(rtol) > 0.0:
            raise ValueError("rtol must be positive, got %r" % (rtol,))
        torch = kde._torch()
        with N.on_device(self.device, stream):
            cd = self._stage_cands(cands, (3, 4))
            lead = tuple(int(v) for v in cd.shape[:-1])
            C = int(np.prod(lead[1:], dtype=np.int64))  # S requests: the flattened pool
            ws = self._workspace(workspace, self.workspace_bytes_logpdf(C),
                                 "B * C = %d * %d exceeds int32" % (self.B, C))
            ll = torch.empty((self.B, C), dtype=torch.float64, device=self.device) if which != "bad" else None
            lg = torch.empty((self.B, C), dtype=torch.float64, device=self.device) if which != "good" else None
            status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            launched = self.B > 0 and C > 0
            if launched:
                N.check(N.lib().hbx_kde_logpdf_groups(*(self.model_args() + (
                    N.ptr(cd), C, float(rtol), LOGPDF_FP64_ONLY if fp64_only else 0, N.ptr(ll), N.ptr(lg),
                    N.ptr(status), N.ptr(ws), ws.numel(), N.stream_handle(stream, self.device)))))
            if not sync:
                return GroupLogPdf(ll, lg, status, None, lead)
            stats = np.zeros(4, dtype=np.int64)
            if launched:
                N.check(N.lib().hbx_kde_logpdf_groups_stats(N.ptr(ws), stats.ctypes.data))
            elif stream is not None:
                stream.synchronize()
            return GroupLogPdf(None if ll is None else ll.cpu().numpy(), None if lg is None else lg.cpu().numpy(),
                               status.cpu().numpy(), stats, lead)

    def workspace_bytes_get_config(self, C, requests=1, masked=False):
        """``masked``: of the call with a request mask or ``skip_random`` (hbx_kde_propose_groups_m)"""
        if masked:
            return int(N.lib().hbx_kde_propose_groups_m_workspace_bytes(self.B, int(requests), int(C), self.D))
        return int(N.lib().hbx_kde_propose_groups_workspace_bytes(self.B, int(requests), int(C), self.D))

    def _get_config_m(self, C, S, requests, seed, levels, rf, bandwidth_factor, counter_base, stream, stream_id,
                      workspace, sync, keep_pools, records, want, skip_random):
        """get_config under a request mask and / or skip_random: one hbx_kde_propose_groups_m call"""
        torch = kde._torch()
        with N.on_device(self.device, stream):
            wd = request_mask(want, self.B, S, self.device)
            ws = self._workspace(workspace, self.workspace_bytes_get_config(C, S, masked=True),
                                 "get_config: B=%d S=%d C=%d out of range (C >= 1, B * S * C within int32)" %
                                 (self.B, S, C))
            lvd = _levels_dev(levels, self.D, self.device)
            rows = torch.empty((self.B * S, self.D), dtype=torch.float64, device=self.device)
            source = torch.empty(self.B * S, dtype=torch.uint8, device=self.device)
            rec = torch.empty((self.B * S, kde.RESULT_BYTES), dtype=torch.uint8, device=self.device) if records else None
            # (the pools of unanswered requests are not written: NaN rather than what the allocation held)
            cands = torch.full((self.B, S, C, self.D), float("nan"), dtype=torch.float64, device=self.device) \
                if keep_pools else None
            N.check(N.lib().hbx_kde_propose_groups_m(*(
                self.model_args() + (N.ptr(lvd), float(bandwidth_factor), rf) + _philox(seed, counter_base, stream_id) +
                (S, C, N.ptr(wd), PROPOSE_SKIP_RANDOM if skip_random else 0, N.ptr(rows), N.ptr(source), N.ptr(rec),
                 N.ptr(cands), N.ptr(ws), ws.numel(), N.stream_handle(stream, self.device),
                 None if self._rules is None else ctypes.addressof(self._rules)))))
            err = None
            if keep_pools:
                off = np.zeros(5, dtype=np.int64)
                N.check(N.lib().hbx_kde_propose_groups_m_ws_offsets(self.B, S, C, self.D, off.ctypes.data))
                err = ws[int(off[1]):int(off[1]) + self.B * S * C].clone().view(self.B, S, C)
                if requests is None:
                    cands, err = cands.view(self.B, C, self.D), err.view(self.B, C)
            return _configs(rows, source, self.B, None if requests is None else S, sync, rec, cands, err)

    def get_config(self, C, seed, levels, requests=None, random_fraction=1.0 / 3, bandwidth_factor=3, counter_base=0,
                   stream=None, stream_id=0, workspace=None, sync=True, keep_pools=False, records=True, want=None,
                   skip_random=False):
        """The reference's get_config (bohb.py:104-169) for ``requests`` requests of every group in one call
        (hbx_kde_propose_groups: ``sample`` with pool size S * C, ``acquire_requests`` and ``finish`` on one stream):
        always a configuration -- the best of the request's C candidates, or a prior draw where the group has no
        model, where the random fraction takes the request, where the sampler met a domain error and where no
        candidate has a score.  ``levels`` may be an int32 device tensor (no upload).  Returns GroupConfigs: rows
        [B, S, D] (``requests`` None: one request, [B, D]); with ``sync=False`` everything stays on the device and
        nothing synchronises.  ``records=False`` leaves ``picks`` None; ``keep_pools`` also returns the pools and
        the sampler's error bytes (``cands`` [B, S, C, D], ``domain_err`` [B, S, C]).

        ``want`` (request_mask's forms: a bool / uint8 mask [B, S], or int counts [B]) and ``skip_random`` make it one
        hbx_kde_propose_groups_m call: only the wanted requests are sampled, scored and finished, each with exactly
        the bytes of the call without a mask; the others come back as SOURCE_SKIPPED with a NaN row and an ACQ_SKIPPED
        record.  ``skip_random``: requests that the random fraction takes are not sampled and scored either -- rows
        and sources are unchanged, their records are skipped ones and their pools are not written (NaN with
        ``keep_pools``).  ``request_stats(workspace)`` reports what was computed."""
        torch = kde._torch()
        S = 1 if requests is None else int(requests)
        C = int(C)
        rf = _fraction(random_fraction)
        if want is not None or skip_random:
            return self._get_config_m(C, S, requests, seed, levels, rf, bandwidth_factor, counter_base, stream,
                                      stream_id, workspace, sync, keep_pools, records, want, bool(skip_random))
        with N.on_device(self.device, stream):
            ws = self._workspace(workspace, self.workspace_bytes_get_config(C, S),
                                 "get_config: B=%d S=%d C=%d out of range (C >= 1, B * S * C within int32)" %
                                 (self.B, S, C))
            lvd = _levels_dev(levels, self.D, self.device)
            rows = torch.empty((self.B * S, self.D), dtype=torch.float64, device=self.device)
            source = torch.empty(self.B * S, dtype=torch.uint8, device=self.device)
            rec = torch.empty((self.B * S, kde.RESULT_BYTES), dtype=torch.uint8, device=self.device) if records else None
            cands = torch.empty((self.B, S, C, self.D), dtype=torch.float64, device=self.device) if keep_pools else None
            self._call("hbx_kde_propose_groups", *(
                self.model_args() + (N.ptr(lvd), float(bandwidth_factor), rf) + _philox(seed, counter_base, stream_id) +
                (S, C, N.ptr(rows), N.ptr(source), N.ptr(rec), N.ptr(cands), N.ptr(ws), ws.numel(),
                 N.stream_handle(stream, self.device))))
            err = None
            if keep_pools:
                off = np.zeros(4, dtype=np.int64)
                N.check(N.lib().hbx_kde_propose_groups_ws_offsets(self.B, S, C, self.D, off.ctypes.data))
                err = ws[int(off[1]):int(off[1]) + self.B * S * C].clone().view(self.B, S, C)
                if requests is None:
                    cands, err = cands.view(self.B, C, self.D), err.view(self.B, C)
            return _configs(rows, source, self.B, None if requests is None else S, sync, rec, cands, err)

    def finish(self, cands, records, domain_err, levels, random_fraction=1.0 / 3, seed=0, counter_base=0, stream=None,
               stream_id=0, sync=True, want=None):
        """The finish step alone (hbx_kde_finish_groups) over caller-made pools: ``cands`` [B, S, C, D] (or [B, C, D])
        float64, ``records`` the ``sync=False`` output of ``acquire_requests`` (or ``acquire``) over them, or None
        (every request SOURCE_NO_MODEL), ``domain_err`` the sampler's error bytes [B, S, C] (or [B, C]), or None.
        ``seed``, ``counter_base`` and ``stream_id`` are the sampler's.  Returns GroupConfigs without picks.
        ``want`` (request_mask's forms): hbx_kde_finish_groups_m -- SOURCE_SKIPPED and a NaN row where it is 0."""
        torch = kde._torch()
        rf = _fraction(random_fraction)
        with N.on_device(self.device, stream):
            cd = self._stage_cands(cands, (3, 4))
            S = None if cd.dim() == 3 else int(cd.shape[1])
            C = int(cd.shape[-2])
            Q = self.B * (1 if S is None else S)
            if C < 1:
                raise N.HbxError("finish: a pool needs at least one candidate")
            if records is not None:
                if not _is_tensor(records) or records.dtype != torch.uint8 or not records.is_contiguous() or \
                        records.numel() != Q * kde.RESULT_BYTES:
                    raise N.HbxError("records must be the contiguous uint8 device tensor of %d records" % Q)
            ed = domain_err
            if ed is not None:
                if not _is_tensor(ed):
                    ed = torch.from_numpy(np.ascontiguousarray(ed, dtype=np.uint8)).to(self.device)
                if ed.dtype != torch.uint8 or not ed.is_contiguous() or ed.numel() != Q * C:
                    raise N.HbxError("domain_err must be contiguous uint8 with one byte per candidate")
            wd = request_mask(want, self.B, 1 if S is None else S, self.device)
            rows, source = _finish(self.device, stream, self.B, S, C, self.D, records, cd, ed, levels, rf, seed,
                                   counter_base, stream_id, wd)
            return _configs(rows, source, self.B, S, sync)

    def propose(self, C, seed, levels, bandwidth_factor=3, counter_base=0, stream=None, requests=None, topk=None):
        """sample + acquire: (rows [B, D] host float64 -- NaN where a group has no pick --, GroupPicks).
        With ``requests=S``: sample + acquire_requests, (rows [B, S, D], GroupPicks of shape [B, S]).
        With ``topk=k``: sample + acquire_topk, (rows [B, k, D] -- NaN rows past a group's count --, GroupTopK);
        not together with ``requests``."""
        if topk is not None:
            if requests is not None:
                raise N.HbxError("propose: topk and requests cannot be combined")
            cands, _ = self.sample(C, seed, levels, bandwidth_factor, counter_base, stream=stream)
            top = self.acquire_topk(cands, topk, stream=stream)
            return top.rows(cands), top
        if requests is None:
            cands, _ = self.sample(C, seed, levels, bandwidth_factor, counter_base, stream=stream)
            picks = self.acquire(cands, stream=stream)
        else:
            cands, _ = self.sample(C, seed, levels, bandwidth_factor, counter_base, stream=stream, requests=requests)
            picks = self.acquire_requests(cands, stream=stream)
        return picks.rows(cands), picks


def group_sizes(lens, D, min_points=None, top_n_percent=15):
    """Per-group (n_good, n_bad) of the BOHB split (kde.split_sizes(..., 'bohb')), 0 / 0 where the reference
    builds no model (bohb.py:234-237); host int64 arrays."""
    mp = int(D) + 1 if min_points is None else int(min_points)
    ng = np.zeros(len(lens), dtype=np.int64)
    nb = np.zeros(len(lens), dtype=np.int64)
    for b, n in enumerate(lens):
        s = kde.split_sizes(int(n), int(D), mp, top_n_percent, "bohb")
        if s is not None:
            ng[b], nb[b] = s
    return ng, nb


def _impute_view(Xd, segd, order, ngd, nbd, ng, nb, B, D, levels, seed, counter, stream_id, device, sh):
    """fit_groups' imputed view of the raw rows (hbx_kde_impute_groups): every group's n_good good rows, then its
    n_bad bad rows, NaN entries filled.  Returns the view's (Xd, segd, seg_h, order, Ntot) and the ``raw`` dict of
    what the model keeps beside it (raw_X, raw_seg_off, raw_order, src_rows, impute_counts)."""
    torch = kde._torch()
    L = N.lib()
    view_h = np.concatenate(([0], np.cumsum(np.where(ng > 0, ng + nb, 0)))).astype(np.int64)
    Nv = int(view_h[-1])
    Xv = torch.zeros((max(Nv, 1), D), dtype=torch.float64, device=device)
    order_v = torch.zeros(max(Nv, 1), dtype=torch.int64, device=device)
    src = torch.zeros(max(Nv, 1), dtype=torch.int32, device=device)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=device)
    viewd = _to_device(view_h, torch.int64, device)
    if B and Nv:
        wb = int(L.hbx_kde_impute_groups_workspace_bytes(Nv, B, D))
        iws = torch.empty(wb, dtype=torch.uint8, device=device)
        N.check(L.hbx_kde_impute_groups(
            N.ptr(Xd), D, N.ptr(segd), B, N.ptr(order), N.ptr(ngd), N.ptr(nbd),
            N.ptr(_levels_dev(levels, D, device)), N.ptr(viewd), Nv, *(_philox(seed, counter, stream_id) + (
                N.ptr(Xv), N.ptr(order_v), N.ptr(src), N.ptr(counts), N.ptr(iws), wb, sh))))
    raw = dict(raw_X=Xd, raw_seg_off=segd, raw_order=order, src_rows=src[:Nv], impute_counts=counts)
    return (Xv, viewd, view_h, order_v, Nv), raw


def fit_groups(X, losses, seg_off, var_type, min_points=None, top_n_percent=15, device=None, stream=None,
               min_bandwidth=None, pdf_floor=N.PDF_FLOOR_DEFAULT, impute_seed=None, levels=None, impute_counter=0,
               impute_stream_id=0):
    """Refit every bracket's good / bad KDE in one batched call (hbx_seg_argsort_ex in numpy's order, then
    hbx_kde_fit), everything kept on the device.  ``X`` [N, D], ``losses`` [N] and ``seg_off`` [B + 1] are host
    arrays or device tensors; ``min_points`` defaults to D + 1 (BOHB's).  ``min_bandwidth`` (None = 0: no clip):
    every fitted bandwidth becomes ``np.clip(bw, min_bandwidth, None)`` where the fit stores it; ``pdf_floor``: the
    floor f of the score max(f, g)/max(l, f) the model's acquisitions form (default 1e-8, the reference snapshot's).
    Returns a GroupModel, which carries both.

    Conditional search spaces: with ``impute_seed`` (and ``levels``, D level counts, 0: continuous) the rows may hold
    NaN at inactive dims.  The argsort is taken on the original losses, then every group's good and bad rows are
    imputed into a view (hbx_kde_impute_groups; Philox counters ``impute_counter`` + view row under
    ``impute_stream_id``) and the fit runs on the view.  The model then holds the view in ``X``, ``seg_off``,
    ``seg_host`` and ``order`` -- a group's segment is its n_good imputed good rows, then its n_bad imputed bad rows
    -- so every grouped call works as it is; the originals are kept in ``raw_X``, ``raw_seg_off``, ``raw_order``,
    with ``src_rows`` (int32 [Nv]: the original local row of each view row) and ``impute_counts`` (int32 [B, 2]:
    entries filled from donors / from the prior).  ``impute_seed`` None: nothing of this happens."""
    pdf_floor, min_bandwidth = N.check_pdf_floor(pdf_floor), N.check_min_bandwidth(min_bandwidth)
    if impute_seed is not None and levels is None:
        raise N.HbxError("fit_groups: impute_seed needs levels (D level counts, 0: continuous)")
    torch = kde._torch()
    L = N.lib()
    D = len(var_type)
    if device is None:
        device = X.device if _is_tensor(X) else kde.default_device()
    seg_h = np.ascontiguousarray((seg_off.cpu().numpy() if _is_tensor(seg_off) else np.asarray(seg_off)),
                                 dtype=np.int64).reshape(-1)
    if seg_h.size < 1 or np.any(np.diff(seg_h) < 0):
        raise N.HbxError("seg_off must be a non-decreasing int64 array of B + 1 offsets")
    B = int(seg_h.size - 1)
    lens = np.diff(seg_h)
    Ntot = int(seg_h[-1] - seg_h[0]) if B else 0
    if B and seg_h[0] != 0:
        raise N.HbxError("seg_off[0] must be 0")
    ng, nb = group_sizes(lens, D, min_points, top_n_percent)
    fg = np.array([kde.bandwidth_factor(int(v), D) if v else 0.0 for v in ng], dtype=np.float64)
    fb = np.array([kde.bandwidth_factor(int(v), D) if v else 0.0 for v in nb], dtype=np.float64)
    vt = np.ascontiguousarray(kde.var_type_codes(var_type))
    with N.on_device(device, stream):
        Xd = _to_device(X, torch.float64, device).reshape(-1, D)
        ld = _to_device(losses, torch.float64, device).reshape(-1)
        if int(Xd.shape[0]) < Ntot or int(ld.shape[0]) < Ntot:
            raise N.HbxError("fit_groups: %d rows / %d losses for %d segment entries" % (Xd.shape[0], ld.shape[0], Ntot))
        if int(Xd.shape[0]) == 0:  # every bracket empty: the calls still want non-null pointers (never read)
            Xd = torch.zeros((1, D), dtype=torch.float64, device=device)
            ld = torch.zeros(1, dtype=torch.float64, device=device)
        segd, ngd, nbd, fgd, fbd, vtd = (_to_device(a, t, device) for a, t in (
            (seg_h, torch.int64), (ng, torch.int64), (nb, torch.int64), (fg, torch.float64), (fb, torch.float64),
            (vt, torch.int32)))
        order = torch.empty(max(Ntot, 1), dtype=torch.int64, device=device)
        bwg = torch.full((B, D), float("nan"), dtype=torch.float64, device=device)
        bwb = torch.full((B, D), float("nan"), dtype=torch.float64, device=device)
        nlg = torch.zeros((B, D), dtype=torch.int32, device=device)
        nlb = torch.zeros((B, D), dtype=torch.int32, device=device)
        sh = N.stream_handle(stream, device)
        if B and Ntot:
            sb = int(L.hbx_sort_scratch_bytes(Ntot))
            scr = torch.empty(sb, dtype=torch.uint8, device=device)
            N.check(L.hbx_seg_argsort_ex(N.ptr(ld), N.ptr(segd), B, int(lens.max()), Ntot, N.ptr(order), N.ptr(scr),
                                         sb, N.ORDER_NUMPY, sh))
        raw = {}
        if impute_seed is not None:  # the fit, and everything after it, sees the imputed view
            (Xd, segd, seg_h, order, Ntot), raw = _impute_view(
                Xd, segd, order, ngd, nbd, ng, nb, B, D, levels, impute_seed, impute_counter, impute_stream_id,
                device, sh)
        if B and Ntot:
            fit = (N.ptr(Xd), D, N.ptr(segd), B, N.ptr(order), N.ptr(ngd), N.ptr(nbd), N.ptr(fgd),
                   N.ptr(fbd), N.ptr(vtd), N.ptr(bwg), N.ptr(bwb), N.ptr(nlg), N.ptr(nlb), sh)
            if min_bandwidth == 0.0:  # no clip: the call as it has always been
                N.check(L.hbx_kde_fit(*fit))
            else:
                r = N.rules(pdf_floor, min_bandwidth)
                N.check(L.hbx_kde_fit_r(*(fit + (ctypes.addressof(r),))))
    return GroupModel(B=B, D=D, var_type=var_type, device=device, X=Xd, losses=ld, seg_off=segd, seg_host=seg_h,
                      order=order, n_good=ng, n_bad=nb, has_model=(ng > 0), n_good_dev=ngd, n_bad_dev=nbd,
                      fac_good_dev=fgd, fac_bad_dev=fbd, vt_dev=vtd, bw_good=bwg, bw_bad=bwb, nlev_good=nlg,
                      nlev_bad=nlb, pdf_floor=pdf_floor, min_bandwidth=min_bandwidth, **raw)


def sort_conditions(conditions, levels):
    """The conditions of a conditional space -- ``(child_dim, parent_dim, allowed_levels)`` each; a child with several
    is active when all hold -- checked and sorted topologically for hbx_rows_deactivate: (child int32[n], parent
    int32[n], allowed uint64[n]) with every condition of a dim ahead of those the dim is the parent of.  HbxError for
    a dim out of range, a parent that is not categorical with at most 64 levels, a level outside the parent's, and
    a cycle."""
    levels = np.asarray(levels, dtype=np.int64)
    D = int(levels.shape[0])
    conds = []
    for cond in conditions:
        c, p, allowed = int(cond[0]), int(cond[1]), [int(a) for a in cond[2]]
        if not (0 <= c < D and 0 <= p < D) or c == p:
            raise N.HbxError("condition (%d, %d): dims must be two different dims in [0, %d)" % (c, p, D))
        if not 0 < levels[p] <= 64:
            raise N.HbxError("condition (%d, %d): a parent must be categorical with at most 64 levels (dim %d has "
                             "levels=%d; conditions on continuous parents are not supported)" % (c, p, p, levels[p]))
        if not allowed or min(allowed) < 0 or max(allowed) >= levels[p]:
            raise N.HbxError("condition (%d, %d): allowed levels %r outside [0, %d)" % (c, p, allowed, levels[p]))
        conds.append((c, p, sum(1 << a for a in set(allowed))))
    parents = {}
    for c, p, _ in conds:
        parents.setdefault(c, []).append(p)
    depth, on_path = {}, set()

    def depth_of(d):
        if d in depth:
            return depth[d]
        if d in on_path:
            raise N.HbxError("conditions form a cycle through dim %d" % d)
        on_path.add(d)
        depth[d] = 1 + max(depth_of(p) for p in parents[d]) if d in parents else 0
        on_path.discard(d)
        return depth[d]

    conds.sort(key=lambda t: depth_of(t[0]))  # (stable: the given order among equals)
    return (np.array([c for c, _, _ in conds], dtype=np.int32), np.array([p for _, p, _ in conds], dtype=np.int32),
            np.array([a for _, _, a in conds], dtype=np.uint64))


def deactivate_rows(rows, child, parent, allowed, stream=None):
    """hbx_rows_deactivate over a contiguous float64 device tensor [..., D], in place; ``child`` / ``parent`` /
    ``allowed``: device tensors of sort_conditions' arrays (allowed as int64 bit patterns)."""
    D = int(rows.shape[-1])
    n = int(rows.numel()) // D
    N.check(N.lib().hbx_rows_deactivate(N.ptr(rows), n, D, N.ptr(child), N.ptr(parent), N.ptr(allowed),
                                        int(child.shape[0]), N.stream_handle(stream, rows.device)))
    return rows


class GroupBOHB(object):
    """B independent BOHB optimisers advancing in lockstep (config #5's workload): what stands in for the reference's
    ``BOHB`` config generator when every run reports the same number of results per step.  ``new_results`` is
    bohb.py:171-251 for all runs at once (one batched refit), ``get_configs`` bohb.py:104-169 for S requests of
    every run (one call, every row on the device).  Run b's observations of a budget are the rows ``[b, :, :]`` of
    that budget's device store; ``kde_models`` maps budget -> GroupModel.  ``var_type``: the KDE's kinds ('c' / 'u'
    per dim), ``levels``: D level counts (0: continuous).

    Conditional search spaces: with ``impute_seed`` the reported rows may hold NaN at inactive dims, and every refit
    imputes them (fit_groups) on a counter block of its own -- ``impute_counter``, which advances by the view's row
    count per refit and is separate from ``counter``.  ``conditions``, a list of ``(child_dim, parent_dim,
    allowed_levels)``: every row ``get_configs`` returns, prior draws included, passes through hbx_rows_deactivate,
    so it holds NaN exactly at its inactive dims."""

    def __init__(self, B, var_type, levels, min_points_in_model=None, top_n_percent=15, num_samples=64,
                 random_fraction=1.0 / 3, bandwidth_factor=3, seed=0, device=None, min_bandwidth=None,
                 pdf_floor=N.PDF_FLOOR_DEFAULT, impute_seed=None, conditions=None, skip_random=False):
        self.B, self.var_type, self.D = int(B), var_type, len(var_type)
        if not isinstance(skip_random, (bool, np.bool_)):
            raise ValueError("skip_random must be a bool, got %r" % (skip_random,))
        self.skip_random = bool(skip_random)  # get_configs' default: random requests are not sampled and scored
        # the acquisition rules every refit and get_config of this optimiser uses (fit_groups)
        self.min_bandwidth, self.pdf_floor = N.check_min_bandwidth(min_bandwidth), N.check_pdf_floor(pdf_floor)
        # (named only where they differ from the reference snapshot's: the refit call is then the one it always was)
        self._rules_kw = {}
        if self.min_bandwidth != 0.0:
            self._rules_kw["min_bandwidth"] = self.min_bandwidth
        if self.pdf_floor != N.PDF_FLOOR_DEFAULT:
            self._rules_kw["pdf_floor"] = self.pdf_floor
        self.levels = np.ascontiguousarray(np.asarray(levels, dtype=np.int32))
        if self.levels.shape != (self.D,):
            raise N.HbxError("levels must have %d entries" % self.D)
        mp = self.D + 1 if min_points_in_model is None else int(min_points_in_model)
        self.min_points_in_model = max(mp, self.D + 1)  # bohb.py:55-57
        self.top_n_percent = top_n_percent
        self.num_samples = int(num_samples)
        self.random_fraction = _fraction(random_fraction)
        self.bandwidth_factor = bandwidth_factor
        self.seed = int(seed)
        self.device = kde.default_device() if device is None else device
        self.configs, self.losses = {}, {}  # budget -> device store [B, n, D] / [B, n]
        self.kde_models = {}
        self.counter = 0  # the next call's Philox counter base
        self._lvd = None
        self.impute_seed = None if impute_seed is None else int(impute_seed)
        self.impute_counter = 0  # the next refit's imputation counter base
        self.conditions = sort_conditions(conditions, self.levels) if conditions else None
        self._cond_dev = None

    def _dev(self, a, shape_tail):
        t = _to_device(a, kde._torch().float64, self.device)
        if t.dim() != 1 + len(shape_tail) + 1 or int(t.shape[0]) != self.B or tuple(t.shape[2:]) != shape_tail:
            raise N.HbxError("expected [%d, m%s], got %s" % (self.B, "".join(", %d" % v for v in shape_tail),
                                                             tuple(t.shape)))
        return t

    def new_results(self, budget, X, losses):
        """m finished runs per optimiser on ``budget``: ``X`` [B, m, D] (the configurations' vectors) and ``losses``
        [B, m], host arrays or device tensors; a crashed run's loss is +inf (bohb.py:189-194).  Returns True when
        the budget's model was refit.  With an ``impute_seed`` the rows may hold NaN at inactive dims; without one a
        host array that holds a NaN is refused (a device tensor is not read back to look)."""
        torch = kde._torch()
        if self.impute_seed is None and not _is_tensor(X) and np.isnan(np.asarray(X, dtype=np.float64)).any():
            raise N.HbxError("new_results: rows hold NaN (inactive dims of a conditional space?): give the "
                             "optimiser an impute_seed")
        Xd, ld = self._dev(X, (self.D,)), self._dev(losses, ())
        if int(Xd.shape[1]) != int(ld.shape[1]):
            raise N.HbxError("new_results: %d rows and %d losses per run" % (Xd.shape[1], ld.shape[1]))
        if budget not in self.configs:  # bohb.py:198-200
            self.configs[budget] = torch.empty((self.B, 0, self.D), dtype=torch.float64, device=self.device)
            self.losses[budget] = torch.empty((self.B, 0), dtype=torch.float64, device=self.device)
        if max(list(self.kde_models.keys()) + [-np.inf]) > budget:  # bohb.py:204-205: a bigger model exists
            return False
        self.configs[budget] = torch.cat((self.configs[budget], Xd), dim=1)
        self.losses[budget] = torch.cat((self.losses[budget], ld), dim=1)
        n = int(self.configs[budget].shape[1])
        if n <= self.min_points_in_model + 1:  # bohb.py:216-217
            return False
        kw = dict(self._rules_kw)
        if self.impute_seed is not None:
            kw.update(impute_seed=self.impute_seed, levels=self._levels(), impute_counter=self.impute_counter)
        gm = fit_groups(self.configs[budget].reshape(self.B * n, self.D), self.losses[budget].reshape(-1),
                        np.arange(self.B + 1, dtype=np.int64) * n, self.var_type, self.min_points_in_model,
                        self.top_n_percent, device=self.device, **kw)
        if self.impute_seed is not None:  # a fresh counter block per refit: one counter per view row
            self.impute_counter += int(gm.seg_host[-1])
        if not np.all(gm.has_model):  # bohb.py:234-237: the previous model, if any, stays
            return False
        self.kde_models[budget] = gm
        return True

    def _levels(self):
        if self._lvd is None:
            self._lvd = kde._torch().from_numpy(self.levels).to(self.device)
        return self._lvd

    def get_configs(self, budget, S=1, counter_base=None, sync=True, want=None, counts=None, skip_random=None):
        """S configurations for every optimiser (``budget`` is the budget they are scheduled for; as in the
        reference, the model of the largest modelled budget answers, bohb.py:124): GroupConfigs with rows
        [B, S, D].  Prior draws while there is no model.  ``counter_base`` None: the internal counter, which
        advances by B * S * num_samples per call.

        ``want`` (a bool / uint8 mask [B, S]) or ``counts`` (ints [B]: run b's first counts[b] requests), host arrays
        or device tensors: only those requests are computed, with the bytes they have without a mask; the others are
        SOURCE_SKIPPED with NaN rows.  The counters advance as without a mask.  ``skip_random`` (None: the
        optimiser's): requests the random fraction takes are not sampled and scored; rows and sources do not change."""
        S = int(S)
        if want is not None and counts is not None:
            raise ValueError("get_configs: give want or counts, not both")
        if counts is not None:
            want = counts
            if not _is_tensor(counts):
                want = np.asarray(counts)
                if want.ndim != 1 or want.dtype.kind not in "iu":
                    raise N.HbxError("counts must be ints [%d], got %s %s" % (self.B, want.dtype, want.shape))
                want = want.astype(np.int64)  # (uint8 counts are counts here, not a mask)
            elif counts.dim() != 1:
                raise N.HbxError("counts must be ints [%d], got %s" % (self.B, tuple(counts.shape)))
        if want is not None:
            with N.on_device(self.device):
                want = request_mask(want, self.B, S, self.device)  # (refusals before the counter moves)
        skip = self.skip_random if skip_random is None else bool(skip_random)
        if counter_base is None:
            counter_base = self.counter
            self.counter += self.B * S * self.num_samples
        dsync = sync and self.conditions is None  # with conditions the rows are deactivated before they leave
        if not self.kde_models:  # bohb.py:109
            cfg = sample_prior(self.B, S, self._levels(), self.seed, counter_base, C=self.num_samples,
                               device=self.device, sync=dsync, want=want)
        else:
            gm = self.kde_models[max(self.kde_models.keys())]
            cfg = gm.get_config(self.num_samples, self.seed, self._levels(), requests=S,
                                random_fraction=self.random_fraction, bandwidth_factor=self.bandwidth_factor,
                                counter_base=counter_base, sync=dsync, want=want, skip_random=skip)
        if self.conditions is None:
            return cfg
        if self._cond_dev is None:
            torch = kde._torch()
            self._cond_dev = tuple(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device)
                                   for a in self.conditions)
        with N.on_device(self.device):
            deactivate_rows(cfg.rows, *self._cond_dev)
            if not sync:
                return cfg
            return _configs(cfg.rows.reshape(-1, self.D), cfg.source.reshape(-1), self.B, S, True,
                            None if cfg.picks is None else cfg.picks.reshape(-1, kde.RESULT_BYTES))


# ---- grouped successive halving ---------------------------------------------------------------------------------
SRC_NONE = -2 ** 31  # include/hbx.h hbx_sh_advance_groups: an empty slot's src (its row is NaN)


def advance(rows, seg_off, mask, K, fresh=None, stream=None, sync=True, device=None, out=None):
    """The next stage of B brackets from their promotion masks (hbx_sh_advance_groups; HB_iteration.py:184-188,
    :135-138).  ``rows`` [N, D] float64, ``seg_off`` [B + 1] int64 and ``mask`` [N] uint8 or bool (any non-zero byte
    is set; what ``promote.promote_segments(..., on_device=True)`` returns), ``fresh`` None or [B, F, D] float64 --
    host arrays or contiguous device tensors.  Per bracket: the rows of its set positions in ascending position, then
    ``fresh[b][0 .. f_b)`` while slots are left, then NaN rows.  Returns ``(rows [B, K, D] float64, src [B, K] int32,
    counts [B, 2] int64)``: ``src`` is the position relative to the bracket's start, ``-1 - i`` for fresh row i and
    SRC_NONE for a NaN row; ``counts[b]`` is (set bytes -- also where they exceed K --, fresh rows used).  Host arrays,
    or with ``sync=False`` device tensors and no synchronisation when every input is a device tensor already.
    ``out``: the three output tensors to write instead of new ones."""
    torch = kde._torch()
    K = int(K)
    if device is None:
        device = rows.device if _is_tensor(rows) else kde.default_device()
    with N.on_device(device, stream):
        rd = _to_device(rows, torch.float64, device, True, "advance: rows")
        sd = _to_device(seg_off, torch.int64, device, True, "advance: seg_off")
        md = _to_device(mask, torch.uint8, device, True, "advance: mask")
        if rd.dim() != 2 or sd.dim() != 1 or int(sd.shape[0]) < 1 or md.dim() != 1 or \
                int(md.shape[0]) != int(rd.shape[0]):
            raise N.HbxError("advance: rows [N, D], seg_off [B + 1] and mask [N] expected, got %s, %s, %s" %
                             (tuple(rd.shape), tuple(sd.shape), tuple(md.shape)))
        B, D = int(sd.shape[0]) - 1, int(rd.shape[1])
        fd, F = None, 0
        if fresh is not None:
            fd = _to_device(fresh, torch.float64, device, True, "advance: fresh")
            if fd.dim() != 3 or int(fd.shape[0]) != B or int(fd.shape[2]) != D:
                raise N.HbxError("advance: fresh must be [%d, F, %d], got %s" % (B, D, tuple(fd.shape)))
            F = int(fd.shape[1])
            if F == 0:
                fd = None
        if out is None:
            ro = torch.empty((B, max(K, 0), D), dtype=torch.float64, device=device)
            so = torch.empty((B, max(K, 0)), dtype=torch.int32, device=device)
            co = torch.zeros((B, 2), dtype=torch.int64, device=device)
        else:
            ro, so, co = out
        N.check(N.lib().hbx_sh_advance_groups(N.ptr(rd), D, N.ptr(sd), B, N.ptr(md), N.ptr(fd), F, K, N.ptr(ro),
                                              N.ptr(so), N.ptr(co), N.stream_handle(stream, device)))
        if not sync:
            return ro, so, co
        if stream is not None:
            stream.synchronize()
        return ro.cpu().numpy(), so.cpu().numpy(), co.cpu().numpy()


class GroupStage(object):
    """What GroupSuccessiveHalving.step hands to the next stage, all on the device: ``rows`` [B, K, D], ``src``
    [B, K] and ``counts`` [B, 2] (``advance``'s), ``fills`` (the GroupConfigs of the reserved fill block, None when
    no run had a deficit) and ``counter_base`` (the block's first Philox counter)."""
    __slots__ = ("rows", "src", "counts", "fills", "counter_base")

    def __init__(self, rows, src, counts, fills, counter_base):
        self.rows, self.src, self.counts, self.fills, self.counter_base = rows, src, counts, fills, counter_base


class GroupSuccessiveHalving(object):
    """One Hyperband bracket of every run of a GroupBOHB, in lockstep (HB_iteration.py:149-190 and, with
    ``resampling_rate``, :203-250 for all B runs at once).  ``num_configs`` / ``budgets``: the bracket's ladder
    (HB_master.hb_bracket / hb_budgets).  Lockstep: a stage's requests are all answered by the model as it stands
    when the stage starts, and its results are reported together -- in the reference the behaviour of a pool with at
    least ``num_configs[stage]`` workers."""

    FILLS = ("all", "needed")

    def __init__(self, num_configs, budgets, resampling_rate=None, min_samples_advance=1, ties="numpy", fills="all"):
        if fills not in self.FILLS:
            raise ValueError("fills must be 'all' or 'needed', got %r" % (fills,))
        self.fills = fills  # 'needed': the fill call computes run b's first K - survivors_b requests only
        self.num_configs = [int(v) for v in num_configs]
        self.budgets = [float(v) for v in budgets]
        if not self.num_configs or len(self.num_configs) != len(self.budgets):
            raise ValueError("num_configs and budgets must have one entry per stage, got %d and %d" %
                             (len(self.num_configs), len(self.budgets)))
        if min(self.num_configs) < 1:
            raise ValueError("every stage needs at least one configuration, got %r" % (self.num_configs,))
        if resampling_rate is not None and not 0.0 <= float(resampling_rate) <= 1.0:
            raise ValueError("resampling_rate must be in [0, 1], got %r" % (resampling_rate,))
        self.resampling_rate = None if resampling_rate is None else float(resampling_rate)
        self.min_samples_advance = min_samples_advance
        N.order_mode(ties)
        self.ties = ties

    def threshold(self, stage):
        """k of the promotion after ``stage``: configurations ranked below it advance (HB_iteration.py:180, :242)."""
        nxt = self.num_configs[stage + 1]
        if self.resampling_rate is None:
            return nxt
        return max(self.min_samples_advance, nxt * (1 - self.resampling_rate))

    def step(self, opt, rows, losses, stage):
        """The transition behind ``stage``: ``rows`` [B, num_configs[stage], D] (a device tensor) ran on
        ``budgets[stage]`` and gave ``losses`` [B, num_configs[stage]] (a non-finite loss is a crashed run).
        Reports them (``opt.new_results``: the reference's new_result per job, before process_results) and, on the
        last stage, returns None (the reference's cleanup).  Otherwise ranks every run's finite losses
        (hbx_sh_promote_ex, numpy's tie order by default), reads ONE pair of scalars back -- the smallest and largest
        advancing count, 16 bytes: the only host read of a transition, it decides whether the fill call is made --,
        asks ``opt.get_configs(budgets[stage + 1], S=K)`` for the fills when a run has fewer than
        K = num_configs[stage + 1] survivors, and compacts (``advance``).  Returns a GroupStage.

        Counters: every transition reserves B * K * num_samples Philox counters of ``opt.counter``, whether the fill
        call runs or not, and fill slot i of run b is request (b, i) of that block: run b's draws depend on (B, b,
        the ladder) only, never on the other runs' data."""
        torch = kde._torch()
        from . import promote
        stage = int(stage)
        if not 0 <= stage < len(self.num_configs):
            raise ValueError("stage %r outside [0, %d)" % (stage, len(self.num_configs)))
        B, n, D = (int(v) for v in rows.shape)
        if B != opt.B or n != self.num_configs[stage] or tuple(losses.shape) != (B, n):
            raise N.HbxError("step: stage %d takes rows [%d, %d, D] and losses [%d, %d], got %s and %s" %
                             (stage, opt.B, self.num_configs[stage], opt.B, self.num_configs[stage],
                              tuple(rows.shape), tuple(losses.shape)))
        opt.new_results(self.budgets[stage], rows, losses)
        if stage == len(self.num_configs) - 1:
            return None
        K = self.num_configs[stage + 1]
        ld = opt._dev(losses, ())
        seg = np.arange(B + 1, dtype=np.int64) * n
        mask, nadv = promote.promote_segments(ld.reshape(-1), seg, np.full(B, self.threshold(stage), dtype=np.float64),
                                              device=opt.device, ties=self.ties, on_device=True)
        lo_hi = torch.stack((nadv.min(), nadv.max())).cpu()  # the transition's one host read: 16 bytes
        base = opt.counter
        opt.counter += B * K * opt.num_samples
        fills = None
        if int(lo_hi[0]) < K:
            # 'needed': run b uses its first K - nadv[b] fill requests and only those are computed (a device tensor of
            # counts: nothing more is read back); same counters, same bytes at every slot that `advance` reads
            kw = dict(counts=(K - nadv.to(torch.int64)).clamp(min=0, max=K)) if self.fills == "needed" else {}
            fills = opt.get_configs(self.budgets[stage + 1], S=K, counter_base=base, sync=False, **kw)
        seg_d = torch.from_numpy(seg).to(opt.device)
        out, src, counts = advance(rows.reshape(B * n, D), seg_d, mask, K, fresh=None if fills is None else fills.rows,
                                   sync=False, device=opt.device)
        return GroupStage(out, src, counts, fills, base)


class GroupStageRecord(object):
    """One stage of one Hyperband iteration, for all B runs: ``iteration``, ``stage``, ``budget``, ``rows`` [B, n, D],
    ``losses`` [B, n], ``src`` [B, n] int32 (``advance``'s map into the previous stage: a position there, or -1 - i
    for fill request i; at stage 0 every row is request i of the iteration's get_configs call: -1 - i) and
    ``model_based`` [B, n] bool (the reference's info_dict['model_based_pick'], carried forward with the row)."""
    __slots__ = ("iteration", "stage", "budget", "rows", "losses", "src", "model_based")

    def __init__(self, iteration, stage, budget, rows, losses, src, model_based):
        self.iteration, self.stage, self.budget = int(iteration), int(stage), float(budget)
        self.rows, self.losses, self.src, self.model_based = rows, losses, src, model_based

    def _to_host(self):
        for name in ("rows", "losses", "src", "model_based"):
            setattr(self, name, getattr(self, name).cpu().numpy())


class GroupRunResult(object):
    """What GroupHyperband.run returns: ``stages`` (the GroupStageRecords in run order; empty with ``keep=None``),
    ``result[(iteration, stage)]`` and ``incumbent()``."""

    def __init__(self, stages, inc_budget, inc_loss, inc_row):
        self.stages = stages
        self._inc = (inc_budget, inc_loss, inc_row)

    def __getitem__(self, key):
        for r in self.stages:
            if (r.iteration, r.stage) == tuple(key):
                return r
        raise KeyError(key)

    def __len__(self):
        return len(self.stages)

    def incumbent(self):
        """Per run ``(budget [B], loss [B], row [B, D])``: the lowest finite loss at the largest budget that has any
        (the first such row in run order), +inf / -inf budget / a NaN row for a run without a finite loss."""
        return self._inc


class GroupHyperband(object):
    """B independent BOHB / Hyperband runs from end to end on the device: ``opt`` (a GroupBOHB) proposes, a
    GroupSuccessiveHalving per iteration promotes.  The ladder is the reference's (HB_master.py:93-94, :161-168).
    Lockstep: a stage's requests are all answered by the model as it stands when the stage starts -- the reference
    with at least as many workers as the stage has configurations.  ``sh_kwargs`` go to GroupSuccessiveHalving
    (``resampling_rate``, ``min_samples_advance``, ``ties``, ``fills``)."""

    def __init__(self, opt, eta=3, min_budget=0.01, max_budget=1, **sh_kwargs):
        from .HB_master import hb_budgets
        if not eta > 1 or not 0 < min_budget <= max_budget:
            raise ValueError("eta > 1 and 0 < min_budget <= max_budget expected, got %r, %r, %r" %
                             (eta, min_budget, max_budget))
        self.opt, self.eta = opt, eta
        self.max_SH_iter, self.budgets = hb_budgets(eta, min_budget, max_budget)
        self.sh_kwargs = sh_kwargs
        GroupSuccessiveHalving([1], [max_budget], **sh_kwargs)  # (argument errors now, not at the first iteration)
        self.iterations = 0  # Hyperband iterations run so far

    def ladder(self, it):
        """(num_configs, budgets) of iteration ``it``."""
        from .HB_master import hb_bracket
        s, ns = hb_bracket(it, self.eta, self.max_SH_iter)
        return ns, [float(b) for b in self.budgets[(-s - 1):]]

    def run(self, n_iterations, objective, keep="host"):
        """``n_iterations`` more Hyperband iterations.  Iteration ``it`` starts with ``opt.get_configs(budgets[0],
        S=ns[0])``; every stage calls ``objective(rows [B, n, D] device float64, budget, info) -> losses [B, n]`` (a
        device tensor or a host array; a non-finite loss is a crashed run; ``info``: iteration, stage, budget) and
        GroupSuccessiveHalving.step moves on.  ``keep``: 'host' (records as numpy arrays, copied once at the end of
        the run), 'device' (tensors) or None (only the incumbents, as host arrays).  Returns a GroupRunResult."""
        if keep not in ("host", "device", None):
            raise ValueError("keep must be 'host', 'device' or None, got %r" % (keep,))
        torch = kde._torch()
        opt = self.opt
        dev = opt.device
        inc_b = torch.full((opt.B,), float("-inf"), dtype=torch.float64, device=dev)
        inc_l = torch.full((opt.B,), float("inf"), dtype=torch.float64, device=dev)
        inc_r = torch.full((opt.B, opt.D), float("nan"), dtype=torch.float64, device=dev)
        stages = []
        for it in range(self.iterations, self.iterations + int(n_iterations)):
            ns, bud = self.ladder(it)
            sh = GroupSuccessiveHalving(ns, bud, **self.sh_kwargs)
            cfg = opt.get_configs(bud[0], S=ns[0], sync=False)
            rows, mb = cfg.rows, cfg.model_based
            src = (-1 - torch.arange(ns[0], dtype=torch.int32, device=dev)).expand(opt.B, ns[0]).contiguous()
            for stage in range(len(ns)):
                losses = opt._dev(objective(rows, bud[stage], dict(iteration=it, stage=stage, budget=bud[stage])), ())
                if tuple(losses.shape) != (opt.B, ns[stage]):
                    raise N.HbxError("objective returned %s, expected (%d, %d)" % (tuple(losses.shape), opt.B,
                                                                                   ns[stage]))
                if keep is not None:
                    stages.append(GroupStageRecord(it, stage, bud[stage], rows, losses, src, mb))
                # incumbent: the lowest finite loss at the largest budget that has one, first row on ties
                fin = torch.isfinite(losses)
                lf = torch.where(fin, losses, torch.full_like(losses, float("inf")))
                m = lf.min(dim=1).values
                first = torch.argmax((lf == m[:, None]).to(torch.uint8), dim=1)
                better = fin.any(dim=1) & ((inc_b < bud[stage]) | ((inc_b == bud[stage]) & (m < inc_l)))
                inc_b = torch.where(better, torch.full_like(inc_b, bud[stage]), inc_b)
                inc_l = torch.where(better, m, inc_l)
                inc_r = torch.where(better[:, None], rows[torch.arange(opt.B, device=dev), first], inc_r)
                nxt = sh.step(opt, rows, losses, stage)
                if nxt is None:
                    break
                adv = nxt.src >= 0
                mbn = torch.gather(mb, 1, nxt.src.clamp(min=0).long())
                if nxt.fills is not None:
                    fi = (-1 - nxt.src).clamp(min=0, max=ns[stage + 1] - 1).long()
                    mbn = torch.where(adv, mbn, torch.gather(nxt.fills.model_based, 1, fi))
                rows, src, mb = nxt.rows, nxt.src, mbn & (nxt.src != SRC_NONE)
            self.iterations = it + 1
        if keep == "host":
            for r in stages:
                r._to_host()
        if keep == "device":
            return GroupRunResult(stages, inc_b, inc_l, inc_r)
        return GroupRunResult(stages, inc_b.cpu().numpy(), inc_l.cpu().numpy(), inc_r.cpu().numpy())
