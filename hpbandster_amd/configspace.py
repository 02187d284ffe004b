"""Minimal ConfigSpace-compatible configuration space (host side, no compute).

HpBandSter's config generators talk to ``ConfigSpace`` through a handful of calls
(``get_hyperparameters()``, ``hasattr(h, 'choices')``, ``sample_configuration()``,
``Configuration(cs, values).get_array()`` and ``Configuration(cs, vector=v).get_dictionary()``;
see ``hpbandster/config_generators/bohb.py:63-77,110,160,211-212`` in the reference).
ConfigSpace is not installed in this image, so the engine ships this small stand-in with
the same surface and the same vector encoding conventions:

* ``UniformFloatHyperparameter``: vector = (v - lower) / (upper - lower) (log space if ``log``).
* ``UniformIntegerHyperparameter``: encoded through a float range widened by 0.49999 on both
  sides, decoded by rounding (ConfigSpace's convention); no ``choices`` -> BOHB type ``'c'``.
* ``CategoricalHyperparameter``: vector = index into ``choices``; BOHB type ``'u'``.
* ``OrdinalHyperparameter``: vector = index into ``sequence``; no ``choices`` -> type ``'c'``.

Hyperparameters are kept sorted by name, which is the order ConfigSpace uses for
unconditioned spaces, so ``get_array()`` columns line up with ``get_hyperparameters()``.
When the real ``ConfigSpace`` package is importable the engine uses it instead
(see ``hpbandster_amd.config_generators._cs``).

Conditions: ``EqualsCondition(child, parent, value)`` and ``InCondition(child, parent, values)`` through
``add_condition(s)``.  A hyperparameter is active when all of its conditions hold and their parents are
active; an inactive one is NaN in the vector (``sample_configuration``, ``get_array``), absent from
``get_dictionary()`` and refused in ``Configuration(values=...)``.
``util.deactivate_inactive_hyperparameters`` turns any vector into a valid configuration.  The columns stay
sorted by name here; the real ConfigSpace orders a conditioned space topologically (parents first), so the
column order of the two differs for such spaces -- the engine reads the order from ``get_hyperparameters()``
either way.  A space without conditions behaves, RNG consumption included, as it did before conditions
existed.
"""

import math

import numpy as np


class Hyperparameter(object):
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "%s(%r)" % (type(self).__name__, self.name)


class UniformFloatHyperparameter(Hyperparameter):
    def __init__(self, name, lower, upper, default_value=None, log=False):
        super().__init__(name)
        if not lower < upper:
            raise ValueError("lower must be < upper for %s" % name)
        if log and lower <= 0:
            raise ValueError("log-scaled hyperparameter %s needs lower > 0" % name)
        self.lower = float(lower)
        self.upper = float(upper)
        self.log = bool(log)
        self.default_value = default_value

    def _bounds(self):
        if self.log:
            return math.log(self.lower), math.log(self.upper)
        return self.lower, self.upper

    def _transform(self, vector_value):
        lo, hi = self._bounds()
        v = vector_value * (hi - lo) + lo
        return math.exp(v) if self.log else float(v)

    def _inverse_transform(self, value):
        lo, hi = self._bounds()
        v = math.log(value) if self.log else float(value)
        return (v - lo) / (hi - lo)

    def _sample_vector(self, rng):
        return rng.uniform()


class UniformIntegerHyperparameter(UniformFloatHyperparameter):
    def __init__(self, name, lower, upper, default_value=None, log=False):
        Hyperparameter.__init__(self, name)
        self.int_lower = int(lower)
        self.int_upper = int(upper)
        self.lower = lower - 0.49999
        self.upper = upper + 0.49999
        self.log = bool(log)
        if log:
            self.lower = max(self.lower, 1e-12)
        self.default_value = default_value

    def _transform(self, vector_value):
        v = int(round(super()._transform(vector_value)))
        return min(max(v, self.int_lower), self.int_upper)


class CategoricalHyperparameter(Hyperparameter):
    def __init__(self, name, choices, default_value=None):
        super().__init__(name)
        self.choices = tuple(choices)
        if len(self.choices) == 0:
            raise ValueError("categorical %s needs at least one choice" % name)
        self.default_value = default_value

    def _transform(self, vector_value):
        return self.choices[int(vector_value)]

    def _inverse_transform(self, value):
        return float(self.choices.index(value))

    def _sample_vector(self, rng):
        return float(rng.randint(len(self.choices)))


class OrdinalHyperparameter(Hyperparameter):
    def __init__(self, name, sequence, default_value=None):
        super().__init__(name)
        self.sequence = tuple(sequence)
        self.default_value = default_value

    def _transform(self, vector_value):
        return self.sequence[int(round(vector_value))]

    def _inverse_transform(self, value):
        return float(self.sequence.index(value))

    def _sample_vector(self, rng):
        return float(rng.randint(len(self.sequence)))


class InCondition(object):
    """``child`` is active only while ``parent`` takes one of ``values``"""

    def __init__(self, child, parent, values):
        self.child, self.parent, self.values = child, parent, tuple(values)
        if not self.values:
            raise ValueError("condition on %s needs at least one value" % parent.name)
        self.vector_values = frozenset(parent._inverse_transform(v) for v in self.values)

    def _holds(self, parent_vector_value):
        return parent_vector_value in self.vector_values  # (False for NaN)

    def __repr__(self):
        return "%s | %s in %r" % (self.child.name, self.parent.name, self.values)


class EqualsCondition(InCondition):
    def __init__(self, child, parent, value):
        super().__init__(child, parent, (value,))
        self.value = value


class ConfigurationSpace(object):
    def __init__(self, seed=None):
        self._hps = {}
        self._conds = {}  # child name -> its conditions
        self.random = np.random.RandomState(seed)

    def add_condition(self, condition):
        c, p = condition.child.name, condition.parent.name
        if self._hps.get(c) is not condition.child or self._hps.get(p) is not condition.parent:
            raise ValueError("condition %r: child and parent must be hyperparameters of this space" % (condition,))
        seen, todo = set(), [p]  # the child must not be an ancestor of its parent
        while todo:
            name = todo.pop()
            if name == c:
                raise ValueError("condition %r closes a cycle" % (condition,))
            if name not in seen:
                seen.add(name)
                todo += [k.parent.name for k in self._conds.get(name, ())]
        self._conds.setdefault(c, []).append(condition)
        return condition

    def add_conditions(self, conditions):
        for c in conditions:
            self.add_condition(c)
        return conditions

    def get_conditions(self):
        return [c for name in sorted(self._conds) for c in self._conds[name]]

    def _active(self, vector):
        """bool per hyperparameter (sorted by name): active under the values of ``vector``"""
        names = self.get_hyperparameter_names()
        pos = {n: i for i, n in enumerate(names)}
        memo = {}

        def active(name):
            if name not in memo:
                memo[name] = all(active(k.parent.name) and k._holds(vector[pos[k.parent.name]])
                                 for k in self._conds.get(name, ()))
            return memo[name]

        return np.array([active(n) for n in names], dtype=bool)

    def seed(self, seed):
        self.random = np.random.RandomState(seed)

    def add_hyperparameter(self, hp):
        if hp.name in self._hps:
            raise ValueError("hyperparameter %s already present" % hp.name)
        self._hps[hp.name] = hp
        return hp

    def add_hyperparameters(self, hps):
        for h in hps:
            self.add_hyperparameter(h)
        return hps

    def get_hyperparameters(self):
        return [self._hps[k] for k in sorted(self._hps)]

    def get_hyperparameter_names(self):
        return sorted(self._hps)

    def get_hyperparameter(self, name):
        return self._hps[name]

    def sample_configuration(self, size=1):
        hps = self.get_hyperparameters()
        out = []
        for _ in range(size):
            vec = np.array([h._sample_vector(self.random) for h in hps], dtype=np.float64)
            if self._conds:  # (every entry is drawn, then the inactive ones are dropped)
                vec[~self._active(vec)] = np.nan
            out.append(Configuration(self, vector=vec))
        return out[0] if size == 1 else out

    def __len__(self):
        return len(self._hps)


class Configuration(object):
    def __init__(self, configuration_space, values=None, vector=None):
        self.configuration_space = configuration_space
        hps = configuration_space.get_hyperparameters()
        if (values is None) == (vector is None):
            raise ValueError("exactly one of values / vector must be given")
        if values is not None and configuration_space._conds:
            vec = np.array([h._inverse_transform(values[h.name]) if h.name in values else np.nan for h in hps],
                           dtype=np.float64)
            act = configuration_space._active(vec)
            missing = [h.name for h, a in zip(hps, act) if a and h.name not in values]
            if missing:
                raise ValueError("missing values for %s" % missing)
            extra = [h.name for h, a in zip(hps, act) if not a and h.name in values]
            if extra:
                raise ValueError("values given for inactive hyperparameters %s" % extra)
            self._vector = vec
        elif values is not None:
            missing = [h.name for h in hps if h.name not in values]
            if missing:
                raise ValueError("missing values for %s" % missing)
            self._vector = np.array([h._inverse_transform(values[h.name]) for h in hps],
                                    dtype=np.float64)
        else:
            vec = np.asarray(vector, dtype=np.float64).reshape(-1)
            if vec.shape[0] != len(hps):
                raise ValueError("vector has %d entries, space has %d" % (vec.shape[0], len(hps)))
            self._vector = np.ascontiguousarray(vec)

    def get_array(self):
        return self._vector

    def get_dictionary(self):
        hps = self.configuration_space.get_hyperparameters()
        if self.configuration_space._conds:  # an inactive hyperparameter has no entry
            return {h.name: h._transform(v) for h, v in zip(hps, self._vector) if v == v}
        return {h.name: h._transform(v) for h, v in zip(hps, self._vector)}

    def __getitem__(self, key):
        return self.get_dictionary()[key]

    def __eq__(self, other):
        return isinstance(other, Configuration) and np.array_equal(self._vector, other._vector)

    def __repr__(self):
        return "Configuration(%r)" % (self.get_dictionary(),)


class util(object):
    """``ConfigSpace.util``, as far as the config generators use it"""

    @staticmethod
    def deactivate_inactive_hyperparameters(configuration, configuration_space, vector=None):
        """The valid Configuration nearest to ``configuration`` (a dict of values) or ``vector``: every
        hyperparameter that is inactive under the others' values is dropped (NaN in the vector)."""
        hps = configuration_space.get_hyperparameters()
        if vector is None:
            vector = [h._inverse_transform(configuration[h.name]) if h.name in configuration else np.nan
                      for h in hps]
        vec = np.array(vector, dtype=np.float64).reshape(-1)
        if vec.shape[0] != len(hps):
            raise ValueError("vector has %d entries, space has %d" % (vec.shape[0], len(hps)))
        vec[~configuration_space._active(vec)] = np.nan
        return Configuration(configuration_space, vector=vec)
