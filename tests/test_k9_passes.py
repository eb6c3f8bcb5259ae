"""The passes word and the entry point of the K9 launch behind `plan` / `plan_star` (batch.k9_passes, batch.k9_entry) against
the expressions the two methods carried before the helper existed, for every combination of the three flags and every
`simplify_passes`.  No GPU."""
import itertools

import pytest

from mopa_rl_amd.batch import BatchPlanner, k9_entry, k9_passes


@pytest.mark.parametrize("vertex_simplify, path_shortcut, path_smooth", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("simplify_passes", [1, 2, 3])
def test_passes_word_and_entry_of_every_flag_combination(vertex_simplify, path_shortcut, path_smooth, simplify_passes):
    # the if / elif chain of `plan` as it stood, written out
    if path_smooth:
        entry, passes = "smooth_paths", 8 | (4 if path_shortcut else 0) | (int(simplify_passes) if vertex_simplify else 0)
    elif path_shortcut:
        entry, passes = "shortcut_paths", 4 | (int(simplify_passes) if vertex_simplify else 0)
    elif vertex_simplify:
        entry, passes = "simplify_paths", simplify_passes
    else:
        entry, passes = None, 0
    assert k9_passes(vertex_simplify, simplify_passes, path_shortcut, path_smooth) == passes
    assert k9_entry(vertex_simplify, path_shortcut, path_smooth) == entry
    assert (passes == 0) == (entry is None), "0 stands for no K9 launch"
    if entry is not None:
        assert callable(getattr(BatchPlanner, entry))
        assert 1 <= passes <= {"simplify_paths": 3, "shortcut_paths": 7, "smooth_paths": 15}[entry], "outside the entry point's range"


def test_the_launch_behind_a_plan_calls_the_selected_entry_with_the_word():
    """`_k9_behind`, the one place `plan` and `plan_star` launch K9 from: the selected method, the word, the planner's own stream
    arguments; nothing when all flags are off"""
    calls = []

    class Spy(BatchPlanner):
        def __init__(self):
            pass

    for name in ("simplify_paths", "shortcut_paths", "smooth_paths"):
        setattr(Spy, name, lambda self, *a, _n=name, **kw: calls.append((_n, a, kw)))
    bp = Spy()
    bp._k9_behind("path", "plen", "status", 7, 3, "ids", "seeds", False, 3, False, False, "s")
    assert calls == []
    bp._k9_behind("path", "plen", "status", 7, 3, "ids", "seeds", True, 2, True, True, "s")
    bp._k9_behind("path", "plen", "status", 7, 3, "ids", "seeds", True, 1, True, False, "s")
    bp._k9_behind("path", "plen", "status", 7, 3, "ids", "seeds", True, 3, False, False, "s")
    common = dict(seed=7, env_id_base=3, env_ids="ids", seeds="seeds", stream="s")
    assert calls == [("smooth_paths", ("path", "plen", "status"), dict(common, passes=14)),
                     ("shortcut_paths", ("path", "plen", "status"), dict(common, passes=5)),
                     ("simplify_paths", ("path", "plen", "status"), dict(common, passes=3))]
