"""aiyagari_hark_amd -- MI355X-native (gfx950) Aiyagari household block.

Drop-in for the hot path of Dostenlinus/Aiyagari-HARK (EGM backward step ->
panel / histogram cross-section -> GE loop).  Compute runs in hand-written HIP
kernels (``csrc/``, built into ``lib/libaiyagari.so`` and called through the C ABI
``include/aiyagari.h``); PyTorch-ROCm only owns device buffers and streams.

The reference's call surface lives in :mod:`aiyagari_hark_amd.model`
(``AiyagariType``, ``AiyagariEconomy``); the batched stationary extensions (GE
bisection on r, Young-lottery histogram, Rouwenhorst) in
:mod:`aiyagari_hark_amd.stationary`; perfect-foresight transition paths after a shock
(``steady_state``, ``household_block``, ``solve_transition``) and the sequence-space Jacobian
of the household block (``household_jacobian``, ``impulse_response``) in
:mod:`aiyagari_hark_amd.transition`; the economy with aggregate TFP risk to first order
(``policy_jacobian``, ``linear_model``, ``simulate``, ``saving_rule``) in
:mod:`aiyagari_hark_amd.aggregate`; wealth statistics of the panel and of histogram
distributions and paths (``histogram_stats``, ``batch_wealth_stats``, ``path_wealth_stats``) and
the same statistics of consumption, income, earnings and cash on hand (``variable_stats``,
``household_variables``, ``batch_inequality``, ``path_variable_stats``) in
:mod:`aiyagari_hark_amd.stats`; values on the histogram and consumption-equivalent welfare gains
(``stationary_value``, ``path_value``, ``welfare.welfare``) in :mod:`aiyagari_hark_amd.welfare`;
cohorts followed through the lotteries and mobility tables (``mobility``, ``cohort_forward``,
``wealth_classes``) in :mod:`aiyagari_hark_amd.mobility`.
"""
from __future__ import annotations

__version__ = "0.1.0"


def __getattr__(name):
    # Lazy: importing the package must not require a GPU (the C ABI loads on first use).
    if name in ("AiyagariType", "AiyagariEconomy", "AggregateSavingRule", "AggShocksDynamicRule",
                "init_Aiyagari_agents", "init_Aiyagari_economy"):
        from . import model
        return getattr(model, name)
    if name in ("steady_state", "household_block", "solve_transition", "TransitionResult", "household_jacobian",
                "HouseholdJacobian", "impulse_response", "path_wealth_stats", "path_variable_stats"):
        from . import transition
        return getattr(transition, name)
    if name in ("policy_jacobian", "PolicyJacobian", "ar1", "linear_model", "AggregateModel", "moments", "expectations",
                "simulate", "AggregateSimulation", "saving_rule"):
        from . import aggregate
        return getattr(aggregate, name)
    if name in ("histogram_stats", "batch_wealth_stats", "WealthStats", "variable_stats", "household_variables",
                "batch_inequality", "VariableStats", "Inequality"):
        from . import stats
        return getattr(stats, name)
    if name in ("welfare", "stationary_value", "path_value", "consumption_equivalent", "WelfareResult"):
        # ``welfare`` is the module (the import binds the name): its function is ``welfare.welfare``
        import importlib
        welfare = importlib.import_module(__name__ + ".welfare")
        return welfare if name == "welfare" else getattr(welfare, name)
    if name in ("mobility", "wealth_classes", "cohorts_by_class", "cohorts_by_state", "cohort_forward",
                "CohortPaths", "MobilityResult"):
        # ``mobility`` is the module (the import binds the name): its function is ``mobility.mobility``
        import importlib
        mobility = importlib.import_module(__name__ + ".mobility")
        return mobility if name == "mobility" else getattr(mobility, name)
    raise AttributeError(name)
