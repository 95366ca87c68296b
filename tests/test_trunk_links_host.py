"""The state machines of the trunk's hand-off objects (functional.IdentityLink / SharedInputLink / BnBwdLink) without a device:
who may take what, once.  (What the kernels do with them: tests/test_gpu_trunk_handoffs.py.)"""
import pytest


@pytest.fixture
def HF():
    from hiast_amd import functional
    return functional


def test_shared_input_give_without_a_taker_keeps_the_gradient(HF):
    link = HF.SharedInputLink()
    assert link.join(gives=True) is False       # the giver's forward: nobody announced itself, it does not take part
    assert link.dx is None and not link.taken


def test_shared_input_take_after_give_returns_it_once_and_a_second_pass_falls_back(HF):
    link = HF.SharedInputLink()
    assert link.join(gives=False) is True and link.join(gives=True) is True     # forward: the taker first, then the giver
    dx = object()
    assert link.give(dx) is None and link.dx is dx          # backward: the giver parks its gradient ...
    assert link.take() is dx and link.dx is None and link.taken                 # ... the taker takes it, once
    assert link.take() is None
    again = object()                                        # second backward over the retained graph: autograd adds the two
    assert link.give(again) is again and link.dx is None and link.take() is None
    assert link.give(None) is None and link.dx is None      # (no data gradient computed: nothing to hand over)


def test_identity_link_is_taken_once(HF):
    link = HF.IdentityLink()
    assert not link.armed and link.take() is None
    link.gated = pair = (object(), object())
    assert link.take() is pair and link.gated is None and link.take() is None


def test_bn_backward_link_deliver_take_discard_on_one_rank(HF, monkeypatch):
    reduced = []

    def from_partial(partial):          # host stand-in of the partial reduction
        reduced.append(partial)
        return ("sums of", partial)
    monkeypatch.setattr(HF.K, "bn_nhwc_stats_from_partial", from_partial)
    monkeypatch.setattr(HF, "_stat_all_reduce", lambda *a, **k: pytest.fail("no exchange on one rank"))
    monkeypatch.setattr(HF, "_stat_wait", lambda *a, **k: pytest.fail("no exchange on one rank"))
    link = HF.BnBwdLink()
    assert link.gate == 0 and link.take() is None           # nobody registered, nothing delivered
    link.register(2, ("x", "mean", "invstd", "gamma", "beta"), 1)
    assert (link.gate, link.world) == (2, 1) and link.saved[0] == "x"
    link.deliver("p0")
    assert link.partial == "p0" and link.sums is None and not reduced          # the partials stay until they are taken
    assert link.take() == ("sums of", "p0") and reduced == ["p0"]
    assert link.partial is None and link.sums is None and link.take() is None   # exactly once
    link.deliver("p1")                  # the BatchNorm's backward was pruned: the next forward drops the leftovers
    link.discard()
    assert link.partial is None and link.sums is None and link.take() is None and reduced == ["p0"]
    assert link.gate == 2               # (the registration is the forward's, not a leftover)
