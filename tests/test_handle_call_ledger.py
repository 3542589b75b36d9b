"""Every public name of _lib.Data has a decision in tests/test_gpu_handle_transitions.py: driven through the chain of calls on one
handle and compared with a fresh handle (COMPARED), called between the compared calls (BETWEEN), or left out with a reason (EXCLUDED).
A new Data method without a decision fails here, without a GPU -- the chain fell behind the class once because nothing said so."""
import inspect
import re

import test_gpu_handle_transitions as chain


def _public_names():
    from ml_amd import _lib
    return sorted(name for name, _ in inspect.getmembers(_lib.Data) if not name.startswith("_"))


def test_every_public_name_of_data_is_in_exactly_one_list():
    lists = {"COMPARED": list(chain.COMPARED), "BETWEEN": list(chain.BETWEEN), "EXCLUDED": list(chain.EXCLUDED)}
    for which, names in lists.items():
        assert len(names) == len(set(names)), "%s names something twice" % which
    listed = [name for names in lists.values() for name in names]
    twice = sorted(name for name in set(listed) if listed.count(name) > 1)
    assert not twice, "in more than one list: %s" % twice
    public = _public_names()
    undecided = sorted(set(public) - set(listed))
    assert not undecided, "Data has public names the handle-transitions chain has no decision for: %s" % undecided
    gone = sorted(set(listed) - set(public))
    assert not gone, "listed, but not a public name of Data: %s" % gone


def test_every_excluded_name_has_a_reason():
    for name, reason in chain.EXCLUDED.items():
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason, name


def test_the_chain_calls_what_it_lists():
    source = inspect.getsource(chain).split("# ---- the ledger", 1)[0]
    for name in chain.COMPARED + chain.BETWEEN:
        assert re.search(r"\.%s\b" % re.escape(name), source), "%s is listed but the chain never calls it" % name
