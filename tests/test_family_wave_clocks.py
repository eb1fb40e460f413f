"""-m gpu: the family launch's wave clocks (ltr_ctx_set_debug "wave_clock", ltr_debug_family_wave_clocks; csrc/ltr_dp_family.hpp):
with the knob on, every wavefront of the family grid records the wall clock at which it started and at which it left, in a buffer of
its own beside the plan kernel's; with the knob off nothing is recorded and the read-back returns 0.  The scores are the same bits
either way."""
import numpy as np
import pytest

from longtr_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _run(ctx, batch, knob):
    try:
        ctx.set_debug("wave_clock", knob)
        plan = ctx.plan(batch)
        plan.execute()
        ll, _ = plan.fetch()
        fam_clocks = plan.family_wave_clocks().copy()
        plan_clocks = plan.wave_clocks().copy() if knob else None
        launches = _lib.debug_last_launches(plan=plan)
        st = plan.family_stats()
        plan.close()
    finally:
        ctx.set_debug("reset", 0)
    return ll, fam_clocks, plan_clocks, launches, st


def test_one_first_and_last_clock_per_wavefront_of_the_family_grid(gpu_ctx):
    loci, _ = synth.config_loci("config3", n_loci=300)
    batch, _ = synth.pack_loci(loci)
    ll_off, clocks_off, _, _, st_off = _run(gpu_ctx, batch, 0)
    ll_on, clocks, plan_clocks, launches, st = _run(gpu_ctx, batch, 1)
    assert st["families"] > 0 and st["families"] == st_off["families"]
    assert clocks_off.shape == (0, 2)                                      # the knob off: the read-back returns 0 wavefronts
    (fam,) = [L for L in launches if L["kind"] == "family"]
    assert clocks.shape == (fam["grid"] * fam["takers"], 2), (clocks.shape, fam)
    first, last = clocks[:, 0], clocks[:, 1]
    assert (first > 0).all() and (first <= last).all()
    span = (int(last.max()) - int(first.min())) / 100.0
    print("family launch: %d wavefronts, first start to last end %.1f us, last ends spread over %.1f us; plan kernel: %d wavefronts"
          % (len(clocks), span, (int(last.max()) - int(last.min())) / 100.0, len(plan_clocks)))
    assert 0 < span < 1e6                                                  # one launch of a 300-locus plan: well under a second of a 100 MHz clock
    assert np.array_equal(ll_on.view(np.uint64), ll_off.view(np.uint64))
