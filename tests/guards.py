"""The one check of the guard elements that core's entry points return for canary > 0 (core._Fresh.guards)."""


def check_guards(guards, guard, names=None, where=None):
    """guards {name: (front, back, pattern)} of a call with canary = guard: the entries are `names` (where given), each
    output has `guard` elements in front and behind and the scratch that many bytes rounded up to 16, and every one of
    them still holds the pattern.  where: the caller's case, for the message."""
    if names is not None:
        assert set(guards) == set(names), (where, sorted(guards), sorted(names))
    for name, (front, back, pattern) in guards.items():
        size = (guard + 15) // 16 * 16 if name == "scratch" else guard
        assert front.size == back.size == size, (where, name, front.size, back.size, size)
        assert (front == pattern).all() and (back == pattern).all(), (where, name, "written outside the tensor")
