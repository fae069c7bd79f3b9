"""The traffic the short-call cases of tests/test_chain_cqpsk_gpu.py run on, judged by the CPU oracle alone (a chain that decodes nothing
equals a reference that holds nothing): at every call size the control-channel capture holds six syncs or more with a good NID, the
voice capture two LDUs or more; at 3201 samples no call brings as many records as the carry holds, at 9600 the new-record count lands on
two or more of carry - 1, carry, carry + 1."""
import numpy as np
import pytest

import orc
import chain_cqpsk_stream as cg
from conftest import golden


@pytest.mark.parametrize("name,n_call", cg.SHORT_CALLS)
def test_short_call_cases_hold_traffic(built, name, n_call):
    iq = np.ascontiguousarray(golden(name)["iq"])
    n_total = (len(iq) // n_call) * n_call
    sym, rec, fl, rows, data = cg.oracle_stream(iq, n_total, n_call)
    nid = [r for r in rows if r[1] == orc.HEV_P25_NID and r[2] > 0]
    assert int(np.count_nonzero(fl & 2)) >= 6 and len(nid) >= 6, (np.count_nonzero(fl & 2), len(nid))
    new = cg.symbols_per_call(iq, n_total, n_call)
    assert new.sum() == len(sym)
    if n_call == 3201:
        assert new.max() < cg.CARRY and n_total // n_call >= 3 * 6
    if n_call == 9600:
        assert len(set(new.tolist()) & {cg.CARRY - 1, cg.CARRY, cg.CARRY + 1}) >= 2, new
    if "_vc" in name:
        ldus = [r for r in nid if r[4] in (5, 10)]
        assert len(ldus) >= 2, nid
        # an LDU's 864 symbols cross three calls or more
        per = np.cumsum(new)
        assert all(np.searchsorted(per, r[0] + 800, side="right") - np.searchsorted(per, r[0], side="right") >= 2 for r in ldus[:-1])
