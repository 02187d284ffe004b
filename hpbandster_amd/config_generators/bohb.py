"""BOHB -- drop-in for hpbandster/config_generators/bohb.py with the KDE work on the MI355X.

Same constructor kwargs, same ``get_config`` / ``new_result`` behaviour and the same consumption of
the global numpy RNG (``np.random.rand`` / ``randint`` and ``scipy.stats.truncnorm.rvs``, in the
reference's order), so a seeded run proposes the same configurations.  What moved to the GPU:

* ``new_result``: the per-budget refit (argsort of the losses, good/bad split, normal-reference
  bandwidths, observed level counts -- bohb.py:220-246) runs in libhbx.so (``kde.fit_pair``);
* ``get_config``: the ``num_samples`` candidates are scored against l (good) and g (bad) and the
  first index of min max(f, g)/max(l, f) (f = ``pdf_floor``, 1e-8 by default) is selected exactly (bohb.py:124-161) by
  ``KDEPair.acquire`` -- fp32 matrix-core scoring of every candidate, fp64 re-score of the ones that
  can still be the minimum.

``kde_models[budget]`` holds a ``KDEPair`` whose ``['good']`` / ``['bad']`` expose ``.data``,
``.bw`` and ``.pdf`` like the statsmodels objects of the reference.
"""

import logging
import threading
import traceback

import numpy as np

from .. import _native
# the host draws (the benchmark reads _HostModel, _draw_rvs, _global_mt, host_draw_ok and _HOSTDRAW from this module)
from ..host_draw import _HOSTDRAW, _MT, _HostModel, _draw_fast, _draw_rvs, _global_mt, host_draw_ok  # noqa: F401
from ..kde import ACQ_DOMAIN_ERR, ObservationStore, mapped_candidates
from .base import base_config_generator
from ._cs import ConfigSpace


class SpeculativeBatch(object):
    """get_config results computed ahead in one batched acquisition (BOHB.get_config_batch_spec).

    The draws were made from a PRIVATE copy of the global RNG: nothing outside changes until a result is
    served.  ``take()`` serves result j only when it is exactly what the sequential call would return at
    that moment -- the model unchanged (``_model_version``), the GPU sampler's counter and the global
    RNG's raw state equal to those before call j -- and then moves the global RNG (under its lock, so no
    other thread's draw can fall between the check and the move) and the counter to where call j leaves
    them.  A random pick (and its warning) is made only when served, from the configspace's own RNG, as
    the sequential call makes it."""

    def __init__(self, gen, entries, states, counters, version):
        self.gen, self.entries, self.states, self.counters, self.version = gen, entries, states, counters, version
        self.mt = _global_mt()
        self.served = 0

    def __len__(self):
        return len(self.entries)

    def _valid_at(self, j):
        gen = self.gen
        return gen._model_version == self.version and gen._sample_counter == self.counters[j]

    def take(self):
        """The next result, or None when it is not the sequential call's (or the batch is used up)."""
        j = self.served
        if j >= len(self.entries) or not self._valid_at(j):
            return None
        mt = self.mt
        with mt.lock:
            if mt.snap() != self.states[j]:
                return None
            mt.load(self.states[j + 1])
        self.gen._sample_counter = self.counters[j + 1]
        self.served += 1
        return self.gen._serve(self.entries[j])

    def continues(self):
        """Every result served and nothing changed since: a longer batch would have stayed valid."""
        j = self.served
        return j == len(self.entries) and self._valid_at(j) and self.mt.snap() == self.states[j]


class BOHB(base_config_generator):
    def __init__(self, configspace, min_points_in_model=None, top_n_percent=15, num_samples=64,
                 random_fraction=1 / 3, bandwidth_factor=3, device=None, sampler="host", sampler_seed=None,
                 speculative="auto", min_bandwidth=None, pdf_floor=_native.PDF_FLOOR_DEFAULT, impute_seed=0,
                 **kwargs):
        super().__init__(**kwargs)
        # conditional search spaces (the configspace reports conditions): an observation holds NaN where a
        # hyperparameter is inactive.  Its store accepts such rows, a refit over rows with a NaN imputes them on the
        # device first (the releases' impute_conditional_data; include/hbx.h hbx_kde_impute_groups) under
        # impute_seed, on the Philox counters [k * cap, ...): k the store's imputing refits so far, cap twice the
        # store's row capacity -- never less than the refit's view rows, and it only grows, so no two refits of a
        # budget share a counter.  Every model-based proposal passes through deactivate_inactive_hyperparameters.
        # A space without conditions reaches none of this.
        self.impute_seed = int(impute_seed)
        self._conditional = bool(getattr(configspace, "get_conditions", lambda: [])())
        self._impute_refits = dict()  # budget -> refits that imputed
        # the two acquisition rules that releases of the package changed after the reference snapshot (include/hbx.h,
        # hbx_rules): min_bandwidth -- every fitted bandwidth becomes np.clip(bw, min_bandwidth, None) (None: no
        # clip, the snapshot's; the releases' constructor default is 1e-3) -- and pdf_floor, the f of the score
        # max(f, g) / max(l, f) (1e-8: the snapshot's; the releases use 1e-32).  Every model this generator fits
        # carries both: its samplers read the clipped bandwidths, its acquisitions form their scores under the floor.
        self.min_bandwidth = _native.check_min_bandwidth(min_bandwidth)
        self.pdf_floor = _native.check_pdf_floor(pdf_floor)
        # speculative batches (SuccessiveHalving serving a stage's back-to-back requests from one batched
        # acquisition): 'auto' = with the GPU sampler only (the host sampler's scipy draws cost ~100x the
        # acquisition, so batching them gains nothing and risks drawing for calls never served),
        # 'always', 'never'
        if speculative not in ("auto", "always", "never"):
            raise ValueError("speculative must be 'auto', 'always' or 'never'")
        self.speculative = speculative
        # sampler 'host': the reference's draws from the global numpy RNG (seeded runs reproduce the
        # reference's proposals); 'gpu': the same rule drawn on the GPU from a Philox stream
        # (distributional parity; for large num_samples, where host sampling dominates)
        if sampler not in ("host", "gpu"):
            raise ValueError("sampler must be 'host' or 'gpu'")
        self.sampler = sampler
        if sampler_seed is None and sampler == "gpu":
            sampler_seed = int.from_bytes(np.random.bytes(8), "little")
        self.sampler_seed = sampler_seed
        self._sample_counter = 0
        self.top_n_percent = top_n_percent
        self.configspace = configspace
        self.bw_factor = bandwidth_factor
        self.min_points_in_model = min_points_in_model
        if min_points_in_model is None:
            self.min_points_in_model = len(self.configspace.get_hyperparameters()) + 1
        self.num_samples = num_samples
        self.random_fraction = random_fraction
        self.device = device

        hps = self.configspace.get_hyperparameters()
        self.kde_vartypes = ""
        self.vartypes = []
        for h in hps:  # bohb.py:69-75
            if hasattr(h, 'choices'):
                self.kde_vartypes += 'u'
                self.vartypes += [len(h.choices)]
            else:
                self.kde_vartypes += 'c'
                self.vartypes += [0]
        self.vartypes = np.array(self.vartypes, dtype=int)
        # engine limits: D <= 256 dims; categorical codes are level indices < 1024 (the
        # level count runs on a 1024-bit map); beyond 64 continuous / 32 categorical dims the KDEs are
        # exact-only (every candidate re-scored in fp64, no fp32 pre-selection)
        if len(self.vartypes) > _native.lib().hbx_max_dims():
            raise ValueError("hpbandster_amd supports at most %d hyperparameters (got %d)"
                             % (_native.lib().hbx_max_dims(), len(self.vartypes)))
        if (self.vartypes > 1024).any():
            raise ValueError("hpbandster_amd supports categorical hyperparameters with at most 1024 choices")

        self.cat_probs = []
        self.configs = dict()
        self.losses = dict()
        self.good_config_rankings = dict()
        self.kde_models = dict()
        self._stores = dict()  # budget -> ObservationStore: the budget's rows resident in HBM
        self._model_version = 0  # bumped whenever kde_models changes (speculative batches check it)
        self._calls = 0  # get_config calls so far
        self._pick_tls = threading.local()  # GPU sampler: this thread's draw / pick buffers (_pick)

    # -- candidates ---------------------------------------------------------------------------
    def sample_candidates(self, kde_good, num_samples, rng=None, out=None):
        """bohb.py:133-147: around a random good observation, truncnorm per continuous dim (bounds
        from bw, scale bandwidth_factor * bw), keep-or-resample per categorical dim.  Global RNG (or
        ``rng``, a RandomState drawn from in the same order).  One native call for every draw of the call
        plus one vectorised truncnorm inversion (``_draw_fast``); the values and the RNG's state after the
        call are the reference's per-element path's bit for bit (``_draw_rvs``, which runs instead when
        host_draw_ok() finds numpy or scipy not as assumed)."""
        R = np.random.mtrand._rand if rng is None else rng
        if host_draw_ok():
            mt = _global_mt() if rng is None else getattr(self, "_rng_mt", (None, None))[1]
            if mt is None or mt.rs is not R:
                try:
                    mt = _MT(R)
                except (TypeError, AttributeError):  # a legacy RandomState over another bit generator (PCG64 ...)
                    mt = None
                if rng is not None and mt is not None:
                    self._rng_mt = (R, mt)
            if mt is not None:
                return _draw_fast(kde_good, self.vartypes, self.bw_factor, num_samples, R, mt, out)
        c = _draw_rvs(kde_good, self.vartypes, self.bw_factor, num_samples, R)
        if out is None:
            return c
        out[...] = c
        return out

    def get_config(self, budget):
        sample = None
        info_dict = {}
        self._calls += 1
        if len(self.kde_models.keys()) == 0 or np.random.rand() < self.random_fraction:
            sample = self.configspace.sample_configuration().get_dictionary()
            info_dict['model_based_pick'] = False

        if sample is None:
            try:
                pair = self._top_pair()
                if self.sampler == "gpu":
                    # one wait: the draws, the acquisition, the domain-error flag and the winning row come back
                    # together (no separate device reduction and row copy)
                    res, best_vector = self._pick(pair, self._sample_counter)
                    self._sample_counter += self.num_samples
                    if res.flags & ACQ_DOMAIN_ERR:
                        raise ValueError("truncnorm domain error: a sampled datum has no valid bounds")
                else:  # drawn into mapped host memory, which the acquisition's kernels read in place
                    cands = self.sample_candidates(pair['good'], self.num_samples,
                                                   out=mapped_candidates(self.num_samples, len(self.vartypes)))
                    res = pair.acquire_mapped(cands)
                    best_vector = cands[res.index].copy() if res.index >= 0 else None
                if res.index < 0:
                    self.logger.debug(self._failed("no score"))
                    sample = self.configspace.sample_configuration().get_dictionary()
                    info_dict['model_based_pick'] = False
                else:
                    if self.logger.isEnabledFor(logging.DEBUG):  # (formatting the vector costs ~0.1 ms)
                        self.logger.debug('best_vector: {}, {}'.format(best_vector, res.score))
                    sample = self._to_dict(best_vector)
                    info_dict['model_based_pick'] = True
            except _native.HbxError:
                raise  # the engine failed: never hide it behind a random configuration
            except Exception:
                self.logger.warning(self._failed("traceback"))
                sample = self.configspace.sample_configuration().get_dictionary()
                info_dict['model_based_pick'] = False
        return sample, info_dict

    def _to_dict(self, vector):
        """A proposed vector as the configuration's dictionary; in a conditional space its inactive hyperparameters
        are dropped first (the model proposes a value in every dim)."""
        if self._conditional:
            return ConfigSpace.util.deactivate_inactive_hyperparameters(
                configuration=None, configuration_space=self.configspace, vector=vector).get_dictionary()
        return ConfigSpace.Configuration(self.configspace, vector=vector).get_dictionary()

    def _top_pair(self):
        """Always the largest budget's model (bohb.py:124): an immutable snapshot, new_result swaps entries."""
        return self.kde_models[max(self.kde_models.keys())]

    def _failed(self, case, then="Using random configuration"):
        """The messages of a model-based call that ends without a pick (bohb.py:155-166), by ``case``: 'traceback'
        (an exception, its traceback included), 'domain' (the GPU sampler's truncnorm domain error) and 'no score'
        (no candidate has a finite score)."""
        head = "Sampling based optimization with %i samples failed" % self.num_samples
        if case == "traceback":
            return "%s\n %s \n%s" % (head, traceback.format_exc(), then)
        if case == "domain":
            return "%s (truncnorm domain error)\n%s" % (head, then)
        return head + " -> using random configuration"

    # -- one GPU-sampler call: draws and acquisition, one wait ----------------------------------------
    def _pick(self, pair, counter):
        """The call's num_samples draws on the Philox `counter` (DeviceKDE.sample into this thread's kept buffers)
        and their acquisition with the pick on the host (KDEPair.acquire_pick with the draws' error flags and the
        winning row): (AcqResult, winning row or None).  Both go straight to their native calls when the thread's
        current device is the model's, each on the thread's current stream."""
        import torch
        dev = pair.good.device
        n, D = self.num_samples, len(self.vartypes)
        t = self._pick_tls
        keep = getattr(t, "keep", None)
        wsb = pair.workspace_bytes(n)
        if keep is None or keep[3].numel() < wsb or keep[0].device != dev:
            keep = t.keep = (torch.empty((n, D), dtype=torch.float64, device=dev),
                             torch.empty(n, dtype=torch.int64, device=dev),
                             torch.empty(n, dtype=torch.uint8, device=dev),
                             torch.empty(wsb, dtype=torch.uint8, device=dev), np.empty(D))
        cands, _, err, ws, row = keep
        pair.good.sample(self.vartypes, self.bw_factor, n, self.sampler_seed, counter, out=keep[:3])
        res = pair.acquire_pick(cands, err, ws, row)
        return res, (row.copy() if res.index >= 0 else None)

    # -- the k best candidates of one pool --------------------------------------------------------
    def get_config_topk(self, budget, k):
        """The k best of ONE pool of num_samples candidates (KDEPair.acquire_topk) instead of get_config's single
        best: ``[(config_dict, {'model_based_pick': True, 'score': s}), ...]`` in ascending (score, candidate
        index) order -- entry 0 is what a model-based get_config returns from the same RNG state.  Fewer than k
        entries when the pool holds fewer candidates with a score; an empty list when there is no model yet or
        the sampling fails (the caller then draws random configurations, as get_config does).

        The candidates are drawn as get_config draws them (sampler 'host': the global numpy RNG; 'gpu': the
        Philox counter), and the RNG is consumed exactly as by one get_config call that goes model-based: its
        random_fraction draw is taken (and ignored: this call is model-based by definition), then the pool."""
        k = int(k)
        if k < 1 or k > 1024:
            raise ValueError("k must be in [1, 1024], got %d" % k)
        if len(self.kde_models.keys()) == 0:
            return []
        np.random.rand()  # get_config's random_fraction draw
        try:
            pair = self._top_pair()
            if self.sampler == "gpu":
                cands, _, err = pair['good'].sample(self.vartypes, self.bw_factor, self.num_samples,
                                                    self.sampler_seed, self._sample_counter)
                self._sample_counter += self.num_samples
                if bool(err.any().item()):
                    raise ValueError("truncnorm domain error: a sampled datum has no valid bounds")
                top = pair.acquire_topk(cands, k)
                rows = cands.cpu().numpy()[top.index]
            else:
                cands = self.sample_candidates(pair['good'], self.num_samples)
                top = pair.acquire_topk(cands, k)
                rows = cands[top.index]
        except _native.HbxError:
            raise  # the engine failed: never hide it
        except Exception:
            self.logger.warning(self._failed("traceback", "No model-based configurations"))
            return []
        return [(self._to_dict(rows[j]), {'model_based_pick': True, 'score': float(top.score[j])})
                for j in range(top.count)]

    # -- several get_config calls in one GPU pass ----------------------------
    def speculation_enabled(self):
        return self.speculative == "always" or (self.speculative == "auto" and self.sampler == "gpu")

    def spec_fingerprint(self):
        """(model version, GPU sampler counter): the same before and after an interval in which no result
        refitted the model.  A hint for SuccessiveHalving's batch sizes only -- every speculative result is
        checked against the full RNG state when served, and a batch cut short by another draw from the
        global RNG drops the sizes back to one."""
        return (self._model_version, self._sample_counter)

    def spec_unchanged(self, fp):
        return fp[0] == self._model_version and fp[1] == self._sample_counter

    def get_config_batch_spec(self, budget, k):
        """k get_config calls drawn and scored now (ONE hbx_kde_acquire_batch pass) from a private copy of
        the global RNG, handed out one at a time by the returned SpeculativeBatch -- each only while it is
        exactly what the sequential call would return at that moment (see SpeculativeBatch).  Returns None
        when the global RNG cannot be copied (not a legacy MT19937 RandomState)."""
        g = _global_mt()
        if g is None:
            return None
        rs = getattr(self, "_spec_rs", None)
        if rs is None:
            rs = self._spec_rs = np.random.RandomState()
            self._spec_mt = _MT(rs)
        pm = self._spec_mt
        states = [g.snap()]
        pm.load(states[0])
        counters = [self._sample_counter]
        version = self._model_version
        entries = self._batch_entries(k, rs, states, counters, pm)
        return SpeculativeBatch(self, entries, states, counters, version)

    def get_config_batch(self, budget, k):
        """``[self.get_config(budget) for _ in range(k)]`` with one GPU pass for all model-based calls.

        Valid while no result arrives in between (the model is fixed): an SH stage's first
        ``num_configs[0]`` samples (HB_iteration.py:136-138).  The global numpy RNG is consumed in the
        same order as k sequential calls (the draws of a call do not depend on earlier calls' scores)
        and the configspace RNG in call order, so the returned list is identical to the sequential one.
        """
        return [self._serve(e) for e in self._batch_entries(k, np.random.mtrand._rand)]

    def _batch_entries(self, k, R, states=None, counters=None, mt=None):
        """The draws of k calls from RandomState R (and the GPU sampler's counter), their candidates scored
        in one batched acquisition.  Per call an entry: ('model', best vector, score) or ('random', log
        level, message) -- the random configuration itself is drawn from the configspace's RNG when the
        entry is served.  With ``states`` / ``counters``: R's raw state (``mt``) and the counter after
        every call are appended."""
        plan = []  # per call: None (random pick), ('err', message) or the row offset of its candidates
        blocks = []
        pair = None
        counter = self._sample_counter
        for _ in range(int(k)):
            if len(self.kde_models.keys()) == 0 or R.rand() < self.random_fraction:
                plan.append(None)
            else:
                if pair is None:
                    pair = self._top_pair()
                if self.sampler == "gpu":
                    plan.append(len(blocks) * self.num_samples)
                    blocks.append(None)
                    counter += self.num_samples
                else:
                    try:  # a sampling error falls back to a random configuration for this call only, after
                        # consuming the RNG exactly as the sequential call would (bohb.py:163-166)
                        block = self.sample_candidates(pair['good'], self.num_samples, rng=R)
                        plan.append(len(blocks) * self.num_samples)
                        blocks.append(block)
                    except Exception:
                        plan.append(("err", self._failed("traceback")))
            if states is not None:
                states.append(mt.snap())
                counters.append(counter)
        entries = []
        if not blocks:
            return [("random", None, None) if p is None else ("random", "warning", p[1]) for p in plan]
        if self.sampler == "gpu":  # one draw for all calls: the same Philox counters as call by call
            cands, _, err = pair['good'].sample(self.vartypes, self.bw_factor, len(blocks) * self.num_samples,
                                                self.sampler_seed, self._sample_counter if states is None
                                                else counters[0])
            if states is None:
                self._sample_counter += len(blocks) * self.num_samples
        else:
            cands, err = np.concatenate(blocks, axis=0), None
        results = pair.acquire_batch(cands, self.num_samples)
        # the winners' rows in one gather (one device-to-host copy for a device candidate set)
        win = [off + results[off // self.num_samples].index for off in plan
               if type(off) is int and results[off // self.num_samples].index >= 0]
        if err is not None:
            import torch
            bad = err.view(len(blocks), self.num_samples).any(dim=1).cpu().numpy()
            rows = cands[torch.as_tensor(win, dtype=torch.int64, device=cands.device)].cpu().numpy() if win else None
        else:
            bad, rows = None, cands[win] if win else None
        w = 0
        for off in plan:
            if off is None:
                entries.append(("random", None, None))
            elif type(off) is tuple:
                entries.append(("random", "warning", off[1]))
            else:
                res = results[off // self.num_samples]
                if bad is not None and bad[off // self.num_samples]:
                    if res.index >= 0:
                        w += 1
                    entries.append(("random", "warning", self._failed("domain")))
                elif res.index < 0:
                    entries.append(("random", "debug", self._failed("no score")))
                else:
                    entries.append(("model", rows[w], res.score))
                    w += 1
        return entries

    def _serve(self, e):
        """One get_config result from a batch entry (the logging and random draws of bohb.py:124-169 happen
        here, when the result is handed out)."""
        if e[0] == "model":
            if self.logger.isEnabledFor(logging.DEBUG):
                self.logger.debug('best_vector: {}, {}'.format(e[1], e[2]))
            return self._to_dict(e[1]), {'model_based_pick': True}
        if e[1] == "warning":
            self.logger.warning(e[2])
        elif e[1] == "debug":
            self.logger.debug(e[2])
        return self.configspace.sample_configuration().get_dictionary(), {'model_based_pick': False}

    # -- observations ---------------------------------------------------------------------------
    def new_result(self, job):
        super().new_result(job)
        if job.result is None:
            loss = np.inf  # crashed runs count as bad configurations (bohb.py:189-192)
        else:
            loss = job.result["loss"]
        budget = job.kwargs["budget"]
        if budget not in self.configs.keys():
            self.configs[budget] = []
            self.losses[budget] = []
        if max(list(self.kde_models.keys()) + [-np.inf]) > budget:  # bohb.py:204-205
            return
        conf = ConfigSpace.Configuration(self.configspace, job.kwargs["config"])
        vec = conf.get_array()
        self.configs[budget].append(vec)
        self.losses[budget].append(loss)
        store = self._stores.get(budget)
        if store is None:
            if self._conditional:
                store = ObservationStore(len(self.kde_vartypes), self.kde_vartypes, device=self.device,
                                         conditional=True)
            else:
                store = ObservationStore(len(self.kde_vartypes), self.kde_vartypes, device=self.device)
            self._stores[budget] = store
        store.add(vec, loss)
        if len(self.configs[budget]) <= self.min_points_in_model + 1:
            return
        # one refit call: the new row to the device, argsort, split, bandwidths, both KDEs prepared
        if self._conditional and store.has_nan:  # the grouped route: rows imputed on the device, then fitted
            k = self._impute_refits.get(budget, 0)
            self._impute_refits[budget] = k + 1
            pair = store.refit(self.min_points_in_model, self.top_n_percent, min_bandwidth=self.min_bandwidth,
                               pdf_floor=self.pdf_floor, impute_seed=self.impute_seed, levels=self.vartypes,
                               impute_counter=k * 2 * store._hcap)
        else:
            pair = store.refit(self.min_points_in_model, self.top_n_percent, min_bandwidth=self.min_bandwidth,
                               pdf_floor=self.pdf_floor)
        if pair is None:  # bohb.py:234-237: too few rows for a KDE
            return
        self.kde_models[budget] = pair  # atomic swap: a concurrent get_config keeps its snapshot
        self._model_version += 1
        if self.logger.isEnabledFor(logging.DEBUG):
            self.logger.debug('done building a new model for budget %f based on %i/%i split\nBest loss for this '
                              'budget:%f\n\n\n\n\n' % (budget, pair.good.nobs, pair.bad.nobs,
                                                           np.min(store.losses_host)))
