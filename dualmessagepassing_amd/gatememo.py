"""Where everything derived from a 0 / 1 gate hangs, and when it is stale -- the one copy of that rule.

A step derives a dozen index arrays from its two ScalarFilter gates (row masks, kept-row lists, kept-edge tiles and CSRs, ...).
Each is built once and shared by every layer, the forward, the backward and the side-stream prefetch, which works only if
every reader looks where every builder left it:

* ``owner``: the layers hand their kernels reshaped views of the gate they were given (a new tensor object per layer); flags
  and memo hang on the tensor those views share (same memory, same version counter).
* ``memo``: an entry hits while its holder's ``_version`` is the one it was made at and every key is the SAME object.
* no entry may reference its own holder (through its keys or its value): the cycle would leave the step's device memory to the
  garbage collector.

Pure Python; imports nothing of the package.
"""

_MEMO = "_dmp_gate_memo"
# flag -> (the attribute it is kept under on the owner, its value where nobody marked it)
_FLAGS = {"binary": ("_dmp_binary", False), "zero_rows": ("_dmp_zero_rows", False), "dense": ("_dmp_dense_gate", False),
          "ones_prefix": ("_dmp_ones_prefix", 0)}


def owner(t):
    """The tensor the views of ``t`` share: its base when ``t`` covers the whole of it (same address, same number of elements),
    else ``t`` itself (a slice says something else than its base; an object that is no tensor is its own owner)."""
    base = getattr(t, "_base", None)
    if base is not None and base.data_ptr() == t.data_ptr() and base.numel() == t.numel():
        return base
    return t


def mark(gate, binary=None, zero_rows=None, dense=None, ones_prefix=None):
    """What the maker of ``gate`` knows about it (None: left as it is).  ``binary``: exactly 0.0 / 1.0, so its row mask says
    everything it says; ``zero_rows``: the rep-net's input rows were multiplied by it, so rows under its zeros are zeros in every
    layer; ``dense``: (almost) all ones, nothing worth skipping; ``ones_prefix``: its first entries are ones by construction."""
    own = owner(gate)
    for name, value in (("binary", binary), ("zero_rows", zero_rows), ("dense", dense), ("ones_prefix", ones_prefix)):
        if value is not None:
            setattr(own, _FLAGS[name][0], value)


def flag(gate, name, resolved=False):
    """The flag ``name`` of ``gate`` as ``mark`` left it on the gate's owner (False / 0 where nobody did).  ``resolved``:
    ``gate`` IS the owner (a getter on the step's host path resolves it once, for its flag reads and its ``memo``)."""
    attr, default = _FLAGS[name]
    return getattr(gate if resolved else owner(gate), attr, default)


def skips_rows(gate, resolved=False):
    """``gate`` is flagged 0 / 1 and not known to be dense: the rows under its zeros are worth leaving out."""
    own = gate if resolved else owner(gate)
    return bool(getattr(own, "_dmp_binary", False) and not getattr(own, "_dmp_dense_gate", False))


def memo(holder, name, keys, build, resolved=False):
    """``build()``, made once per version of ``holder`` (a gate, through its ``owner``; or any object, e.g. a ``GraphIndex``) and
    tuple of ``keys`` (compared by identity).  ``name`` (hashable; a tuple where several entries of a kind live side by side)
    says which product: a miss replaces the entry of that name, a new version of the holder drops all its entries.  A holder
    that cannot carry an attribute gets the value built on every call.  ``build`` None: a miss returns None (``peek``)."""
    own = holder if resolved else owner(holder)
    held = getattr(own, _MEMO, None)
    if held is not None and held[0] == getattr(own, "_version", None):
        hit = held[1].get(name)
        if hit is not None and len(hit[0]) == len(keys):
            for a, b in zip(hit[0], keys):
                if a is not b:
                    break
            else:
                return hit[1]
    if build is None:
        return None
    value = build()
    version, held = getattr(own, "_version", None), getattr(own, _MEMO, None)      # (read again: ``build`` may have stored on ``own``)
    try:
        if held is None or held[0] != version:
            held = (version, {})
            setattr(own, _MEMO, held)
        held[1][name] = (tuple(keys), value)
    except AttributeError:
        pass
    return value


def peek(holder, name, keys=()):
    """The value ``memo`` would return without building, or None."""
    return memo(holder, name, keys, None)


def names(holder):
    """The names of the entries ``holder`` carries at its current version (for a test that says "nothing hangs here")."""
    own = owner(holder)
    held = getattr(own, _MEMO, None)
    return tuple(held[1]) if held is not None and held[0] == getattr(own, "_version", None) else ()


def plant(holder, name, keys, value):
    """``value``, built elsewhere (a batched launch), left where ``memo(holder, name, keys, ...)`` finds it."""
    return memo(holder, name, keys, lambda: value)
