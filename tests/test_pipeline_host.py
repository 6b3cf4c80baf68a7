"""CPU checks of vmatting.pipeline.SlotPipeline.run, the generator FrameStream and ClipStream share: a stub whose
hooks only record their calls (plain objects for slots, no streams) pins the order of the hooks, the lag, what happens
when the source fails, and that an abandoned generator is drained."""

import pytest

DEPTHS = (1, 2, 3)


def make(depth):
    from vmatting.pipeline import SlotPipeline

    class Stub(SlotPipeline):
        def __init__(self):
            self.depth, self.calls = depth, []

        def check_item(self, item):
            self.calls.append(("check", item))
            if item == "bad":
                raise ValueError("bad item")
            return item, 2 * item

        def _setup(self):
            self.calls.append(("setup",))
            self._slots = [object() for _ in range(self.depth)]

        def _begin(self):
            self.calls.append(("begin",))

        def _submit(self, s, index, item, twice):
            assert s is self._slots[index % self.depth] and twice == 2 * item
            s_index[id(s)] = item
            self.calls.append(("submit", index, item))

        def _retire(self, s):
            self.calls.append(("retire", s_index[id(s)]))
            return 10 * s_index[id(s)]

        def _drain(self):
            self.calls.append(("drain",))

    s_index = {}
    return Stub()


def names(p):
    return [c[0] for c in p.calls]


@pytest.mark.parametrize("depth", DEPTHS)
def test_hook_order_and_lag(depth):
    p = make(depth)
    assert p._slots is None
    got = []
    for r in p.run(iter(range(1, 6))):
        got.append(r)
        # the result of item i comes once item i + depth - 1 was submitted (and before the next one is asked for)
        assert [c for c in p.calls if c[0] == "submit"][-1][2] == min(5, r // 10 + depth - 1)
    assert got == [10, 20, 30, 40, 50]
    assert p.calls[:4] == [("check", 1), ("setup",), ("begin",), ("submit", 0, 1)]
    assert names(p).count("setup") == 1 and names(p).count("begin") == 1
    assert p.calls[-1] == ("drain",) and names(p).count("drain") == 1
    # every item: checked, then submitted, then retired; submissions and retirements in source order
    for kind in ("check", "submit", "retire"):
        assert [c[-1] for c in p.calls if c[0] == kind] == [1, 2, 3, 4, 5]
    for i in range(1, 6):
        assert p.calls.index(("check", i)) < p.calls.index(("submit", i - 1, i)) < p.calls.index(("retire", i))
    # the first result lags the source by depth - 1 items
    assert names(p)[:names(p).index("retire")].count("submit") == min(depth, 5)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("bad_item", (False, True))
def test_source_error_after_three_items(depth, bad_item):
    boom = OSError("decoder lost the file")

    def source():
        yield from (1, 2, 3)
        if bad_item:
            yield "bad"
        raise boom
    p = make(depth)
    got = []
    with pytest.raises(ValueError if bad_item else OSError) as e:
        for r in p.run(source()):
            got.append(r)
    assert got == [10, 20, 30]
    if not bad_item:
        assert e.value is boom
    assert names(p).count("retire") == 3 and names(p).count("drain") == 1
    assert names(p).index("drain") > max(i for i, n in enumerate(names(p)) if n == "retire")
    # the object runs again, on the slots it has
    p.calls.clear()
    assert list(p.run([4, 5])) == [40, 50]
    assert "setup" not in names(p) and names(p).count("begin") == 1 and p.calls[-1] == ("drain",)


def test_bad_item_raises_the_check_s_own_exception():
    p = make(2)
    caught = []
    orig = p.check_item

    def check(item):
        try:
            return orig(item)
        except ValueError as e:
            caught.append(e)
            raise
    p.check_item = check
    with pytest.raises(ValueError) as e:
        list(p.run([1, "bad", 3]))
    assert e.value is caught[0] and ("check", 3) not in p.calls


@pytest.mark.parametrize("depth", DEPTHS)
def test_empty_source_touches_nothing(depth):
    p = make(depth)
    assert list(p.run(iter([]))) == []
    assert p.calls == [] and p._slots is None


@pytest.mark.parametrize("depth", DEPTHS)
def test_closing_early_drains_once_and_runs_again(depth):
    p = make(depth)
    g = p.run(iter(range(1, 9)))
    assert next(g) == 10
    g.close()
    assert names(p).count("drain") == 1 and p.calls[-1] == ("drain",)
    p.calls.clear()
    assert list(p.run([6, 7, 8])) == [60, 70, 80]
    assert names(p).count("setup") == 0 and names(p).count("drain") == 1
