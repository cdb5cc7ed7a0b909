"""Strategy masks: which (s, t) connection strategies a render keeps the colour of (cl2_set_strategy_mask).

A pixel-sample of the bidirectional estimator is a sum over strategy pairs (s, t): s = light vertices used (0..6), t = camera
vertices used (1..6), s + t >= 2 -- 41 pairs.  Pair (s, t) owns bit (t - 1) * 7 + s of a 64-bit mask (include/clive2_amd.h:
CL2_STRATEGY_BIT); a path of pair (s, t) has s + t - 1 edges.  A masked pair keeps its MIS weight and loses its colour, so the
pictures of masks that partition ALL add up to the full picture.

Nothing here needs the library or a GPU.  No reference counterpart (src/trace.metal:649-825 sums all pairs).
"""
MAX_S, MAX_T = 6, 6


def is_pair(s, t):
    """(s, t) is one of the 41 strategy pairs"""
    return isinstance(s, int) and isinstance(t, int) and 0 <= s <= MAX_S and 1 <= t <= MAX_T and s + t >= 2


def bit(s, t):
    """The mask bit of pair (s, t): 1 << ((t - 1) * 7 + s).  ValueError for a pair outside the 41."""
    if isinstance(s, bool) or isinstance(t, bool) or not is_pair(s, t):
        raise ValueError(f"({s!r}, {t!r}) is not a strategy pair: s in 0..{MAX_S}, t in 1..{MAX_T}, s + t >= 2")
    return 1 << ((t - 1) * 7 + s)


PAIRS = tuple((s, t) for t in range(1, MAX_T + 1) for s in range(MAX_S + 1) if s + t >= 2)   # in bit order
ALL = sum(bit(s, t) for s, t in PAIRS)


def mask(pairs):
    """The mask of an iterable of (s, t) pairs."""
    m = 0
    for p in pairs:
        try:
            s, t = p
        except (TypeError, ValueError):
            raise ValueError(f"{p!r} is not an (s, t) pair") from None
        m |= bit(s, t)
    return m


def pairs(m):
    """The (s, t) pairs of a mask, in bit order (t outer, s inner: the order in which the kernel adds them).  Bits outside the 41
    are dropped, as cl2_set_strategy_mask drops them."""
    m = int(m)
    return [(s, t) for s, t in PAIRS if m & bit(s, t)]


def path_length(kmin, kmax=None):
    """The mask of the pairs whose paths have kmin..kmax edges (s + t - 1); kmax=None: kmin and longer."""
    if isinstance(kmin, bool) or not isinstance(kmin, int) or kmin < 1:
        raise ValueError("path length: kmin must be an integer >= 1")
    if kmax is not None and (isinstance(kmax, bool) or not isinstance(kmax, int) or kmax < kmin):
        raise ValueError("path length: kmax must be an integer >= kmin, or None")
    return mask((s, t) for s, t in PAIRS if kmin <= s + t - 1 and (kmax is None or s + t - 1 <= kmax))


LIGHT_IMAGE = mask((s, t) for s, t in PAIRS if t == 1)     # what is splatted into the light image (the caustics)
CAMERA_IMAGE = mask((s, t) for s, t in PAIRS if t >= 2)    # what a pixel's own camera path collects

# directly seen emitters, direct light, indirect light
LAYERS = {"emission": path_length(1, 1), "direct": path_length(2, 2), "indirect": path_length(3)}

SINGLETONS = {f"s{s}t{t}": bit(s, t) for s, t in PAIRS}    # render_layers(passes, SINGLETONS) is the pyramid


MAX_LAYERS = 8     # CL2_MAX_LAYERS (include/clive2_amd.h)


def layer_masks(layers):
    """The layer table of cl2_set_layers: {name: mask or pairs} -> the list of masks in the dictionary's order, bits outside the 41
    dropped.  ValueError for more than MAX_LAYERS layers or for layers that share a pair (a pair adds to at most one layer); an
    empty layer and pairs in no layer are fine.  Needs no renderer."""
    items = list(dict(layers).items())
    if len(items) > MAX_LAYERS:
        raise ValueError(f"{len(items)} layers: a layer table holds at most {MAX_LAYERS}")
    out, seen = [], {}
    for name, m in items:
        m = to_mask(m) & ALL
        for s, t in pairs(m):
            if (s, t) in seen:
                raise ValueError(f"layers {seen[(s, t)]!r} and {name!r} share the pair ({s}, {t}): layers must be disjoint")
            seen[(s, t)] = name
        out.append(m)
    return out


def _int(text, what):
    text = text.strip()
    if not text or not text.isdigit():
        raise ValueError(f"{what}: {text!r} is not a non-negative integer")
    return int(text)


def parse_strategies(spec):
    """The mask of "s,t;s,t;..." (render.py --strategies), e.g. "0,2;1,2".  ValueError for anything else."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("strategies: expected \"s,t;s,t;...\"")
    m = 0
    for item in spec.split(";"):
        parts = item.split(",")
        if len(parts) != 2:
            raise ValueError(f"strategies: {item!r} is not \"s,t\"")
        m |= bit(_int(parts[0], "strategies"), _int(parts[1], "strategies"))
    return m


def parse_path_length(spec):
    """The mask of "A" (exactly A edges), "A:B" (A..B edges) or "A:" (A edges and more) (render.py --path-length)."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("path length: expected A, A:B or A:")
    parts = spec.split(":")
    if len(parts) > 2:
        raise ValueError(f"path length: {spec!r} is not A, A:B or A:")
    a = _int(parts[0], "path length")
    if len(parts) == 1:
        return path_length(a, a)
    return path_length(a, None if not parts[1].strip() else _int(parts[1], "path length"))


def to_mask(mask_or_pairs):
    """None -> ALL; an integer -> itself (it must be >= 0); an iterable of (s, t) pairs -> their mask."""
    if mask_or_pairs is None:
        return ALL
    if isinstance(mask_or_pairs, bool):
        raise ValueError("a strategy mask is an integer or an iterable of (s, t) pairs")
    if hasattr(mask_or_pairs, "__index__"):
        m = int(mask_or_pairs)
        if m < 0 or m >= 1 << 64:
            raise ValueError("a strategy mask is a 64-bit unsigned integer")
        return m
    return mask(mask_or_pairs)
