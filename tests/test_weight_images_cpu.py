"""weight_images.ImageSet without a device: the one freshness rule, event by event, and the lease.  The build itself is replaced by
a counter (`_launch` is the one method everything a build enqueues goes through)."""
import pytest
import torch

import fcaf3d_amd.functional as Fn
from fcaf3d_amd import weight_images as WI


class Counting(WI.ImageSet):
    builds = 0

    def _launch(self):
        self.builds += 1


@pytest.fixture
def mode(monkeypatch):
    m = [2]
    monkeypatch.setattr(Fn, 'split_mode', lambda: m[0])       # the getter the key reads (the real one asks the HIP library)
    return m


def _set():
    torch.manual_seed(0)
    return Counting([torch.nn.Parameter(torch.randn(3, 4, 4)) for _ in range(3)])


def test_functional_still_exports_the_table():
    assert Fn.WeightImages is WI.WeightImages


def test_ensure_builds_exactly_when_the_rule_says_so(mode):
    s = _set()
    p = s.sources[1]

    def ensure(lease):
        before = s.builds
        if lease:
            with s.lease():
                built = s.ensure(trusted=WI.ImageSet.held is s)
        else:
            built = s.ensure(trusted=WI.ImageSet.held is s)
        assert built == (s.builds == before + 1) and s.builds - before in (0, 1)
        return built

    assert s.built is None
    assert ensure(lease=True)                     # first ensure
    assert s.built == (0, 2)
    assert not ensure(lease=True)                 # again under a lease
    assert ensure(lease=False)                    # no lease, no static_weights: untrusted callers rebuild every call
    assert ensure(lease=False)
    assert not ensure(lease=True)
    with torch.no_grad():
        p.mul_(2)
    assert ensure(lease=True)                     # the version key moved
    assert not ensure(lease=True)
    p.data.mul_(2)
    assert not ensure(lease=True)                 # the documented blind spot: a write through .data moves no counter ...
    s.invalidate()
    assert s.built is None
    assert ensure(lease=True)                     # ... so the writer says so
    assert not ensure(lease=True)
    mode[0] = 0
    assert ensure(lease=True)                     # the operand split changed: the images are of the other mode
    assert s.built == (1, 0)
    assert not ensure(lease=True)
    assert s.builds == 6


def test_static_weights_callers_pass_their_own_trust(mode):
    """eval mode with static_weights (NetProgram.forward passes trusted=True without a lease): built once, and again after a write"""
    s = _set()
    assert s.ensure(trusted=True) and not s.ensure(trusted=True)
    with torch.no_grad():
        s.sources[0].add_(1)
    assert s.ensure(trusted=True) and not s.ensure(trusted=True)


def test_an_exception_inside_the_lease_withdraws_it(mode):
    s = _set()
    with pytest.raises(ZeroDivisionError):
        with s.lease():
            assert WI.ImageSet.held is s
            1 / 0
    assert WI.ImageSet.held is None
    assert s.ensure(trusted=WI.ImageSet.held is s) and s.ensure(trusted=WI.ImageSet.held is s)      # nobody is trusted any more
    with s.lease():                               # ... and the next step can take it again
        assert not s.ensure(trusted=WI.ImageSet.held is s)


def test_a_second_lease_while_one_is_held_asserts(mode):
    a, b = _set(), _set()
    with a.lease():
        with pytest.raises(AssertionError):
            with b.lease():
                pass
        assert WI.ImageSet.held is a                   # the failed attempt took nothing away
    assert WI.ImageSet.held is None


def test_lookup_serves_only_covered_kernels(mode):
    s = _set()                                    # 4 x 4 kernels are not MFMA-shaped: no images, nothing to look up
    assert s.images.n == 0 and s.lookup(s.sources[0], False) is None
    w = torch.nn.Parameter(torch.zeros(1, 32, 64))             # forward image only: (64, 32) is no tile of the backward-data launch
    s = Counting([w])
    with s.lease():
        assert s.lookup(w, False) is s.images.table[(w.data_ptr(), 1, 32, 64)][0] and s.lookup(w, True) is None
