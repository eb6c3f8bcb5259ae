"""gjk_distance's contract on the device (k_geom_sep_exact through batch.geom_sep(exact=True)): the pairs whose distance is a formula
(gjk_cases.py), with their swapped forms, one launch per band.  The truth bounds of test_gjk_truth_host are asserted on the device
values directly, and the values have the bits of the host form."""
import numpy as np
import pytest

import frames_ref as F
import gjk_cases as G
import proximity_exact_ref as X
import proximity_ref as P
from geom_ref import MESH
from test_gjk_truth_host import _bits, check_truth

pytestmark = pytest.mark.gpu


def test_device_values_satisfy_the_truth_bounds():
    import torch
    from mopa_rl_amd.batch import geom_sep
    from mopa_rl_amd.scene import load_scene
    can = P.can_of(load_scene("sawyer_lift_obstacle"))
    its = list(G.items(can))
    its += [it._replace(case=it.case.swapped(), form=it.form + ", swapped") for it in its if it.case.t2 != MESH]
    cs = [it.case for it in its]
    types, recs = F.recs_of(cs)
    tt, tr, tc = torch.from_numpy(types).cuda(), torch.from_numpy(recs).cuda(), torch.from_numpy(can).cuda()
    assert len(cs) > 12000
    for band in X.BANDS:
        got = geom_sep(tt, tr, band, mesh_verts=tc, exact=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        check_truth(its, got, band, "device")
        want = X.host_sep(cs, can, band)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), (band, [(its[i].family, its[i].form, got[i], want[i]) for i in np.nonzero(bad)[0][:8]])
