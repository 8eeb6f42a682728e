"""Drop-in for ``kpal.kdistlib``: :class:`ProfileDistance` and :func:`distance_matrix`.

The default pipeline of ``ProfileDistance.distance`` -- copy, optional balance, multiset or
euclidean (kpal/kdistlib.py:126-161) -- runs as fused HIP kernels (``kpal_pair_distance``), and
``distance_matrix`` over P profiles is ONE tiled kernel launch (``kpal_distance_matrix``) instead
of P(P-1)/2 Python-level distances; profiles are balanced once each, which is identical to the
reference balancing copies inside every pair.  The optional positive / dynamic-smooth / scale
steps (kpal/kdistlib.py:143-157) and cosine similarity run on the device too
(``kpal_profile_distance``) whenever every callable is one of kPAL's built-ins (the values of
``metrics.summary`` / ``metrics.pairwise`` / ``metrics.vector_distance``, recognised by identity);
a user-supplied callable cannot enter a kernel and keeps the reference's NumPy formulation.

Beyond the reference: :func:`cross_distances` / :func:`cross_distance_matrix` / :func:`nearest` -- the Q x R rectangle of
distances between a left and a right set of profiles (``kpal_cross_distance_device``; with positive / scale / cosine
``kpal_cross_profile_distance_device``; with dynamic smoothing ``kpal_cross_smooth_distance_device``), a fixed number of
launches per chunk of the right side.  :func:`nearest_chunks` / :func:`nearest_profiles` -- the n nearest right profiles of
every left profile without that rectangle on the host (``kpal_cross_nearest_device``: tiled over both sides, finished and
selected on the device), the left side streamed.  :func:`paired_distances` / :func:`successive_distances` -- the distances of the
LINKED pairs of two sets, ``left[i]`` against ``right[i]``, or of one set against itself ``lag`` profiles on
(``kpal_paired_distance_device``, with dynamic smoothing ``kpal_paired_smooth_distance_device``: a number of launches that
does not grow with the number of pairs).  :func:`pooled_nearest` -- every left profile assigned to its nearest right profile and
the left profiles pooled bin by bin (``kpal_pool_groups_device`` on the tables the selection ran on), the left side streamed.
"""
import contextlib

import numpy as np

from . import _native, metrics


def _plain_int64(a):
    return (isinstance(a, np.ndarray) and a.dtype == np.int64 and a.ndim == 1 and a.flags['C_CONTIGUOUS']
            and a.flags['WRITEABLE'])


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


class ProfileDistance(object):
    """Configurable distance between two profiles (kpal/kdistlib.py:21-51)."""

    def __init__(self, do_balance=False, do_positive=False, do_smooth=False,
                 summary=metrics.summary['min'], threshold=0, do_scale=False,
                 down=False, distance_function=None,
                 pairwise=metrics.pairwise['prod']):
        self._do_balance = do_balance
        self._do_positive = do_positive
        self._do_smooth = do_smooth
        self._threshold = threshold
        self._do_scale = do_scale
        self._down = down
        self._distance_function = distance_function
        self._pairwise = pairwise
        self._function = summary

    # ---- dynamic smoothing (kpal/kdistlib.py:53-124) ---------------------------------------------
    def _collapse(self, vector, start, length):
        """Sums of the four quarters of ``vector[start:start+length]``."""
        return np.reshape(vector[start:start + length], (4, length // 4)).sum(axis=1)

    def _dynamic_smooth(self, left, right, start, length):
        if length == 1:
            return
        left_c = self._collapse(left.counts, start, length)
        right_c = self._collapse(right.counts, start, length)
        if min(self._function(left_c), self._function(right_c)) <= self._threshold:
            left.counts[start] = left_c.sum()
            right.counts[start] = right_c.sum()
            left.counts[start + 1:start + length] = 0
            right.counts[start + 1:start + length] = 0
            return
        quarter = length // 4
        for i in range(4):
            self._dynamic_smooth(left, right, start + i * quarter, quarter)

    def dynamic_smooth(self, left, right):
        """Collapse sub-profiles that fail the summary/threshold test, in place
        (kpal/kdistlib.py:112-124).  Built-in summary functions on int64 profiles run as a
        level-wise tree reduction on the GPU; anything else takes the reference's recursion."""
        code = metrics.summary_code(self._function)
        lc, rc = left.counts, right.counts
        if (code is not None and _plain_int64(lc) and _plain_int64(rc) and lc.size == rc.size
                and _is_number(self._threshold)):
            _native.context().dynamic_smooth(lc, rc, left.length, code, self._threshold)
            return
        self._dynamic_smooth(left, right, 0, left.number)

    # ---- routing -------------------------------------------------------------------------------
    def _native_metric(self):
        """Metric code when the final reduction can run on the GPU, else None."""
        if not self._distance_function:
            return metrics.pairwise_code(self._pairwise)
        if self._distance_function is metrics.euclidean:
            return _native.EUCLIDEAN
        if self._distance_function is metrics.cosine_similarity:
            return _native.COSINE
        return None

    def _native_options(self):
        """``kpal_distance_options`` for this configuration, or None if a user-supplied callable
        or a non-numeric threshold keeps it in Python."""
        metric = self._native_metric()
        if metric is None:
            return None
        summary = 0
        if self._do_smooth:
            summary = metrics.summary_code(self._function)
            if summary is None or not _is_number(self._threshold):
                return None
        return _native.DistanceOptions(
            do_balance=int(bool(self._do_balance)), do_positive=int(bool(self._do_positive)),
            do_smooth=int(bool(self._do_smooth)), summary=summary,
            threshold=float(self._threshold) if self._do_smooth else 0.0,
            do_scale=int(bool(self._do_scale)), down=int(bool(self._down)), metric=metric)

    def _is_plain(self):
        return not (self._do_positive or self._do_smooth or self._do_scale)

    def distance(self, left, right):
        """Distance between two profiles; the inputs are left unmodified
        (kpal/kdistlib.py:126-161, tests/test_kdistlib.py:124-135)."""
        metric = self._native_metric()
        dev = _device_pair(left, right)
        if dev is not None:
            # both tables are still in HBM (klib.Profile.from_fasta_by_record): the same kernels on the device copies, no transfer
            ctx, dl, dr = dev
            if self._is_plain() and metric is not None and metric != _native.COSINE:
                return ctx.pair_distance_device(4 ** left.length, dl, dr, metric, do_balance=self._do_balance, k=left.length)
            options = self._native_options()
            if options is not None:
                return ctx.profile_distance_device(left.length, dl, dr, options)
        integer = (np.asanyarray(left.counts).dtype.kind in 'iub' and np.asanyarray(right.counts).dtype.kind in 'iub'
                   and len(left.counts) == len(right.counts))
        if self._is_plain() and metric is not None and metric != _native.COSINE and integer:
            # fused: balanced copies are made on the device, nothing is written back
            return _native.context().pair_distance(left.counts, right.counts, metric,
                                                   do_balance=self._do_balance, k=left.length)
        options = self._native_options() if integer else None
        if options is not None:
            # the whole option pipeline on device copies (kdistlib.py:136-161)
            return _native.context().profile_distance(left.counts, right.counts, left.length, options)

        left = left.copy()
        right = right.copy()
        if self._do_balance:
            left.balance()
            right.balance()
        if self._do_positive:
            left.counts = metrics.positive(left.counts, right.counts)
            right.counts = metrics.positive(right.counts, left.counts)
        if self._do_smooth:
            self.dynamic_smooth(left, right)
        if self._do_scale:
            left_scale, right_scale = metrics.get_scale(left.counts, right.counts)
            if self._down:
                left_scale, right_scale = metrics.scale_down(left_scale, right_scale)
            left.counts = left.counts * left_scale
            right.counts = right.counts * right_scale
        if not self._distance_function:
            return metrics.multiset(left.counts, right.counts, self._pairwise)
        return self._distance_function(left.counts, right.counts)


def distance_matrix(profiles, output, precision, dist):
    """Write the lower-triangular distance matrix of ``profiles`` to ``output``
    (kpal/kdistlib.py:164-186): the count, the names, then row i = distances to profiles
    0..i-1, ``precision`` decimals, space separated."""
    count = len(profiles)
    print(str(count), file=output)
    for profile in profiles:
        print(profile.name, file=output)
    if count < 2:
        return

    metric = dist._native_metric()
    same_k = len(set(p.length for p in profiles)) == 1
    values = _device_matrix(profiles, dist, metric) if same_k else None
    if values is not None:
        _write_matrix(output, count, values, precision)
        return
    integer = all(np.asanyarray(p.counts).dtype.kind in 'iub' for p in profiles)
    options = dist._native_options() if (same_k and integer) else None
    if dist._is_plain() and metric is not None and metric != _native.COSINE and same_k and integer:
        values = _native.context().distance_matrix([p.counts for p in profiles], profiles[0].length, metric,
                                                   do_balance=dist._do_balance)
    elif options is not None and options.do_smooth:
        # gathered once; one pyramid of node sums and codes per profile, every pair through the rectangle kernels
        ctx = _cross_context(profiles)
        with _DeviceSet(ctx, profiles) as pset:
            values = ctx.smooth_distance_matrix_device(count, profiles[0].length, pset.ptr, options)
    elif options is not None:
        # profiles uploaded (and balanced) once, every pair through the option kernels
        values = _native.context().profile_distance_matrix([p.counts for p in profiles], profiles[0].length, options)
    else:
        values = [dist.distance(profiles[i], profiles[j]) for i in range(1, count) for j in range(i)]

    _write_matrix(output, count, values, precision)


#: Right-side tables resident at a time in :func:`cross_distances` unless ``max_bytes`` says otherwise: an eighth of the
#: 288 GB of an MI355X, so the default needs no device query.
CROSS_MAX_BYTES = 32 << 30


def cross_chunks(table_bytes, count, max_bytes):
    """Bounds ``[(start, stop), ...]`` of the chunks ``count`` right-side tables of ``table_bytes`` each are processed in so
    that at most ``max_bytes`` of them are resident at a time -- never less than one table per chunk."""
    per = _chunk_tables(table_bytes, max_bytes)
    return [(at, min(at + per, count)) for at in range(0, count, per)]


def _chunk_tables(table_bytes, max_bytes):
    return max(1, int(max_bytes) // int(table_bytes))


def _chunked(iterable, size):
    chunk = []
    for item in iterable:
        chunk.append(item)
        if len(chunk) == size:
            yield chunk
            chunk = []
    if chunk:
        yield chunk


def _device_table(profile):
    """(context, device address) of the table of ``profile`` while it is in HBM only, else None -- of any object: what has no
    ``_device_counts`` (the profiles of the reference, stand-ins) is not in HBM."""
    at = getattr(profile, '_device_counts', None)
    return at() if at is not None else None


class _DeviceSet(object):
    """The tables of ``profiles`` (one k) as consecutive int64 tables in HBM on ``ctx``: where they lie when they are
    consecutive tables of one batch on that context, otherwise gathered (device-to-device copies for tables in HBM on that
    context, uploads for host counts) into an allocation that ``release`` -- the end of a ``with`` -- frees."""

    def __init__(self, ctx, profiles):
        k = profiles[0].length
        table_bytes = 8 * 4 ** k
        devs = [d if d and d[0] is ctx else None for d in map(_device_table, profiles)]
        self.ctx, self.owned = ctx, None
        first = devs[0]
        if first and all(d and d[1] == first[1] + i * table_bytes for i, d in enumerate(devs)):
            self.ptr = first[1]
            return
        self.ptr = self.owned = ctx.alloc(len(profiles) * table_bytes)
        try:
            for i, (p, d) in enumerate(zip(profiles, devs)):
                if d:
                    ctx.d2d(self.ptr + i * table_bytes, d[1], table_bytes)
                else:
                    ctx.h2d(self.ptr + i * table_bytes, _native._as_i64(p.counts))
        except BaseException:
            self.release()
            raise

    def release(self):
        if self.owned is not None:
            owned, self.owned = self.owned, None
            self.ctx.sync()
            self.ctx.free(owned)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()


def _right_set(ctx, lset, left, right):
    """The device set of ``right`` for a ``with``: ``lset`` itself, which stays its maker's to release, when both sides are
    the same profiles."""
    if len(right) == len(left) and all(a is b for a, b in zip(right, left)):
        return contextlib.nullcontext(lset)
    return _DeviceSet(ctx, right)


def _cross_context(profiles):
    """The context the first device-resident profile lives on, else the default one."""
    for p in profiles:
        d = _device_table(p)
        if d:
            return d[0]
    return _native.context()


def _integer_counts(profile):
    return _device_table(profile) is not None or np.asanyarray(profile.counts).dtype.kind in 'iub'


def cross_distances(left_profiles, right_profiles, dist, max_bytes=None):
    """``values[q, r] = dist.distance(left_profiles[q], right_profiles[r])`` as a float64 array of shape (Q, R).

    A plain ``dist`` (no positive / smooth / scale step, a built-in metric other than cosine) over integer profiles of one k
    is a fixed number of launches per chunk of the right side (``kpal_cross_distance_device``: a rectangle kernel and a
    reduction, a balance per profile with ``do_balance``, a second rectangle kernel when a fast form gives up on the values): the left tables stay resident,
    ``right_profiles`` -- any iterable, read once -- is taken in chunks of at most ``max_bytes`` of tables (default
    ``CROSS_MAX_BYTES``, never less than one table).  Tables that are consecutive in one device batch are used where they
    lie.  Any other ``dist`` made of built-ins -- positive, scale, cosine -- takes the same route through
    ``kpal_cross_profile_distance_device``: each profile balanced once, the masks and the pairs' scale factors applied inside
    the rectangle kernels (one totals pass, or one more rectangle pass for the masked totals of positive + scale), still a
    fixed number of launches per chunk.  So is dynamic smoothing (``kpal_cross_smooth_distance_device``): a node collapses when
    the summary of EITHER partner's quarters is at or below the threshold, a flag per profile, so every profile gets one
    pyramid of node sums and codes and a pair's distance is taken over the bins and nodes live for that pair.  Only positive
    + smoothing (node sums of masked tables depend on the partner), and pyramids past the library's 32 GiB budget, run the pair
    pipeline once per pair inside the library.  A user-supplied callable, a non-numeric threshold, mixed k or non-integer
    counts are ``dist.distance`` pair by pair."""
    left = list(left_profiles)
    if not left:
        raise ValueError('cross_distances needs at least one left profile')
    metric = dist._native_metric()
    k = left[0].length
    plain = dist._is_plain() and metric is not None and metric != _native.COSINE
    options = None if plain else dist._native_options()
    fast = ((plain or options is not None)
            and all(p.length == k for p in left) and all(_integer_counts(p) for p in left))
    if not fast:
        right = list(right_profiles)
        return np.array([[dist.distance(l, r) for r in right] for l in left], dtype=np.float64).reshape(len(left), len(right))
    table_bytes = 8 * 4 ** k
    per = _chunk_tables(table_bytes, CROSS_MAX_BYTES if max_bytes is None else max_bytes)
    ctx = _cross_context(left)
    blocks = []
    with _DeviceSet(ctx, left) as lset:
        for chunk in _chunked(right_profiles, per):
            if any(p.length != k or not _integer_counts(p) for p in chunk):
                # a mixed-k pair raises what dist.distance raises; other counts (scaled profiles) keep its formulation
                blocks.append(np.array([[dist.distance(l, r) for r in chunk] for l in left], dtype=np.float64))
                continue
            with _right_set(ctx, lset, left, chunk) as rset:
                if plain:
                    blocks.append(ctx.cross_distance_device(k, len(left), lset.ptr, len(chunk), rset.ptr, metric,
                                                            do_balance=dist._do_balance))
                elif options.do_smooth:
                    blocks.append(ctx.cross_smooth_distance_device(k, len(left), lset.ptr, len(chunk), rset.ptr, options))
                else:
                    blocks.append(ctx.cross_profile_distance_device(k, len(left), lset.ptr, len(chunk), rset.ptr, options))
    if not blocks:
        return np.zeros((len(left), 0), dtype=np.float64)
    return np.concatenate(blocks, axis=1)


def _paired_options(dist, profiles):
    """The ``kpal_distance_options`` of ``dist`` when the set entries can serve ``profiles`` -- built-ins only, one k, integer
    counts or tables in HBM -- else None."""
    options = dist._native_options()
    if options is None or not profiles:
        return None
    k = profiles[0].length
    if not all(p.length == k and _integer_counts(p) for p in profiles):
        return None
    return options


def paired_distances(left_profiles, right_profiles, dist, max_bytes=None):
    """``values[i] = dist.distance(left_profiles[i], right_profiles[i])`` as a float64 array of shape (N,): what ``kpal
    distance`` prints for two files of N profiles each.  Sides of unequal length raise ``ValueError``.

    With a ``dist`` made of built-ins over integer profiles of one k this is ``kpal_paired_distance_device``: per group of pairs
    one metric kernel over all pairs and one reduction (with scale a totals kernel and its reduction before them, with
    ``do_balance`` one set balance per side), whatever the number of pairs; a pair's value is the same bits in any set, at any
    position.  Tables that are consecutive in one device batch are used where they lie; anything else is gathered (host counts
    uploaded) in groups of at most ``max_bytes`` of tables over both sides (default ``CROSS_MAX_BYTES``, never less than one
    pair).  Dynamic smoothing is ``kpal_paired_smooth_distance_device``: one pyramid of node sums and codes per distinct table
    (k + 1 launches), one metric kernel over the bins and nodes live for each pair and one reduction, whatever the number of
    pairs; only positive + smoothing runs the pair pipeline once per pair inside the library.  A user-supplied callable, a non-numeric
    threshold, mixed k or non-integer counts are ``dist.distance`` pair by pair -- and so is a single pair, which keeps the
    route and the bits of ``dist.distance``."""
    left, right = list(left_profiles), list(right_profiles)
    if len(left) != len(right):
        raise ValueError('paired_distances needs as many left as right profiles ({0} against {1})'.format(len(left), len(right)))
    options = _paired_options(dist, left + right) if len(left) > 1 else None
    if options is None:
        return np.array([dist.distance(l, r) for l, r in zip(left, right)], dtype=np.float64).reshape(len(left))
    k = left[0].length
    per = _chunk_tables(2 * 8 * 4 ** k, CROSS_MAX_BYTES if max_bytes is None else max_bytes)
    ctx = _cross_context(left + right)
    blocks = []
    for at in range(0, len(left), per):
        lgroup, rgroup = left[at:at + per], right[at:at + per]
        with _DeviceSet(ctx, lgroup) as lset, _right_set(ctx, lset, lgroup, rgroup) as rset:
            entry = ctx.paired_smooth_distance_device if options.do_smooth else ctx.paired_distance_device
            blocks.append(entry(k, len(lgroup), lset.ptr, rset.ptr, options))
    return np.concatenate(blocks)


def successive_distances(profiles, dist, lag=1):
    """``values[i] = dist.distance(profiles[i], profiles[i + lag])`` as a float64 array of shape (N - lag,): the compositional
    breakpoint scan over the windows of ``Profile.from_fasta_by_window``.  ``lag < 1`` and ``lag >= N`` raise ``ValueError``.

    Under the conditions of :func:`paired_distances` the profiles are made ONE set (used where they lie when they are consecutive
    tables of one device batch) and the library is given that set and the same set ``lag`` tables on: with ``do_balance`` it
    balances the N tables once, not the two sides of N - ``lag`` each, and with ``do_smooth`` it builds the N pyramids of
    the set once (``kpal_paired_smooth_distance_device``)."""
    profiles = list(profiles)
    lag = int(lag)
    if lag < 1:
        raise ValueError('successive_distances needs lag >= 1')
    if lag >= len(profiles):
        raise ValueError('successive_distances needs more than lag = {0} profiles ({1} given)'.format(lag, len(profiles)))
    pairs = len(profiles) - lag
    options = _paired_options(dist, profiles) if pairs > 1 else None
    if options is None:
        return np.array([dist.distance(profiles[i], profiles[i + lag]) for i in range(pairs)], dtype=np.float64)
    k = profiles[0].length
    ctx = _cross_context(profiles)
    with _DeviceSet(ctx, profiles) as pset:
        entry = ctx.paired_smooth_distance_device if options.do_smooth else ctx.paired_distance_device
        return entry(k, pairs, pset.ptr, pset.ptr + lag * 8 * 4 ** k, options)


def nearest(values, n):
    """For each row of ``values`` the indices of its ``n`` smallest entries, ascending, ties by the lower index, NaN last
    (an int array of shape (rows, min(n, columns)))."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 2:
        raise ValueError('nearest needs a two-dimensional array')
    n = max(0, min(int(n), values.shape[1]))
    return np.argsort(values, axis=1, kind='stable')[:, :n]


def _left_chunks(profiles, max_bytes):
    """Lists of consecutive profiles of the iterable ``profiles`` of at most ``max_bytes`` of tables each (never less than one
    profile).  A chunk that is so far one run of consecutive tables of a device batch ends in front of a device-resident
    profile that does not continue the run: ``_DeviceSet`` then uses the run where it lies.  Reads one profile ahead."""
    chunk, size, run = [], 0, None   # run: (context, address) the next table must have to continue the chunk's run
    for p in profiles:
        nbytes = 8 * 4 ** p.length
        at = _device_table(p)
        if chunk and (size + nbytes > max_bytes or (run is not None and at is not None and at != run)):
            yield chunk
            chunk, size = [], 0
        run = (at[0], at[1] + nbytes) if at is not None and (not chunk or run == at) else None
        chunk.append(p)
        size += nbytes
    if chunk:
        yield chunk


def _merge_nearest(distances, indices, have, values, first, m):
    """Columns ``[0, have)`` of ``distances`` / ``indices`` (every index below ``first``) merged with the block ``values`` of
    right profiles ``first, first + 1, ...`` in the order of :func:`nearest`; returns how many columns are valid now."""
    rows, count = values.shape
    all_d = np.concatenate([distances[:, :have], values], axis=1)
    all_i = np.concatenate([indices[:, :have], np.broadcast_to(np.arange(first, first + count, dtype=np.int64), (rows, count))],
                           axis=1)
    keep = min(m, have + count)
    order = nearest(all_d, keep)    # stable: of equal distances the earlier column, which has the lower index
    distances[:, :keep] = np.take_along_axis(all_d, order, axis=1)
    indices[:, :keep] = np.take_along_axis(all_i, order, axis=1)
    return keep


def nearest_chunks(left_profiles, right_profiles, dist, n, max_bytes=None):
    """The ``n`` nearest of ``right_profiles`` for every profile of ``left_profiles``: a generator of ``(chunk, indices,
    distances)`` -- a list of consecutive left profiles, and for them an int64 and a float64 array of shape ``(len(chunk),
    min(n, R))``: row q holds the positions in ``right_profiles`` of the nearest profiles of ``chunk[q]`` in the order of
    :func:`nearest` (ascending distance, ties by the lower position, NaN last) and ``dist.distance`` to each.

    ``left_profiles`` is any iterable, read once, a chunk of at most ``max_bytes`` of tables (default ``CROSS_MAX_BYTES``, never
    less than one profile) at a time and at most one profile past the chunk being worked on; a chunk is not referenced by the
    generator once the caller has come back for the next one, so the device batches behind the profiles of
    ``Profile.from_fastq_by_record`` are freed as a scan goes.  ``right_profiles`` is a sequence (anything else is made a list):
    when its tables fit ``max_bytes`` they are made resident once for the whole call, otherwise they are taken in chunks of
    that size for every chunk of the left side.

    With a ``dist`` made of built-ins over integer profiles of one k, and ``n <= _native.NEAREST_MAX``, the Q x R distances
    never reach the host: ``kpal_cross_nearest_device`` cuts the rectangle into tiles, finishes every tile's distances on the
    device and keeps the n best of every row there (dynamic smoothing: tile by tile through a host buffer).  A user-supplied
    callable, a non-numeric threshold, mixed k, non-integer counts or a larger ``n`` are ``dist.distance`` pair by pair within
    a chunk and :func:`nearest` over its rows."""
    n = int(n)
    if n < 1:
        raise ValueError('nearest_chunks needs n >= 1')
    if not (hasattr(right_profiles, '__len__') and hasattr(right_profiles, '__getitem__')):
        right_profiles = list(right_profiles)
    return _nearest_chunks(left_profiles, right_profiles, dist, n, CROSS_MAX_BYTES if max_bytes is None else max_bytes)


def _nearest_chunks(left_profiles, right, dist, n, max_bytes, hand_on=False):
    """``hand_on``: yields ``(chunk, indices, distances, left set)`` instead, while the chunk's ``_DeviceSet`` is still
    resident (None where the chunk took no fast route): :func:`pooled_nearest` pools the tables it was made for."""
    R = len(right)
    m = min(n, R)
    options = dist._native_options() if n <= _native.NEAREST_MAX else None
    bounds = cross_chunks(8 * 4 ** right[0].length, R, max_bytes) if R else []
    whole = list(right[0:R]) if len(bounds) == 1 else None    # the right side when it is resident for the whole call
    ctx = whole_set = None
    with contextlib.ExitStack() as whole_call:       # releases the right side that is resident for the whole call
        for chunk in _left_chunks(left_profiles, max_bytes):
            rows, k = len(chunk), chunk[0].length
            distances = np.full((rows, m), np.nan, dtype=np.float64)
            indices = np.full((rows, m), -1, dtype=np.int64)
            fast_left = options is not None and all(p.length == k and _integer_counts(p) for p in chunk)
            have, lset = 0, None
            with contextlib.ExitStack() as this_chunk:   # releases the left set, made when the first block needs it
                for start, stop in bounds:
                    block = whole if whole is not None else list(right[start:stop])
                    if fast_left and all(p.length == k and _integer_counts(p) for p in block):
                        if ctx is None:
                            ctx = _cross_context(chunk)
                        if lset is None:
                            lset = this_chunk.enter_context(_DeviceSet(ctx, chunk))
                        if whole is not None and whole_set is None:
                            whole_set = whole_call.enter_context(_DeviceSet(ctx, whole))
                        with (contextlib.nullcontext(whole_set) if whole is not None else _DeviceSet(ctx, block)) as rset:
                            ctx.cross_nearest_device(k, rows, lset.ptr, stop - start, rset.ptr, options, m, right_first=start,
                                                     have=have, dist=distances, index=indices)
                        have = min(m, have + stop - start)
                    else:
                        # a mixed-k pair raises what dist.distance raises; other counts keep its formulation
                        values = np.array([[dist.distance(l, r) for r in block] for l in chunk], dtype=np.float64)
                        have = _merge_nearest(distances, indices, have, values.reshape(rows, stop - start), start, m)
                    block = None
                if hand_on:
                    yield chunk, indices, distances, lset
            if not hand_on:
                yield chunk, indices, distances
            chunk = lset = None


def nearest_profiles(left_profiles, right_profiles, dist, n, max_bytes=None):
    """:func:`nearest_chunks` over the whole left side: ``(indices, distances)``, an int64 and a float64 array of shape
    ``(Q, min(n, R))``."""
    if not (hasattr(right_profiles, '__len__') and hasattr(right_profiles, '__getitem__')):
        right_profiles = list(right_profiles)
    m = min(max(int(n), 0), len(right_profiles))
    indices, distances = [np.zeros((0, m), dtype=np.int64)], [np.zeros((0, m), dtype=np.float64)]
    for _, i, d in nearest_chunks(left_profiles, right_profiles, dist, n, max_bytes=max_bytes):
        indices.append(i)
        distances.append(d)
    return np.concatenate(indices, axis=0), np.concatenate(distances, axis=0)


def pooled_nearest(left_profiles, right_profiles, dist, max_bytes=None):
    """Assigns every left profile to its nearest right profile and pools the left profiles bin by bin: ``(indices, distances,
    pools)`` -- column 0 of :func:`nearest_profiles` ``(..., 1)`` as an int64 and a float64 array of shape ``(Q,)``, and a list
    of R entries: ``pools[r]`` is the pooled profile (``klib.pooled``) of the left profiles whose nearest is
    ``right_profiles[r]``, named after it, or None where none fell.  A left profile whose nearest distance is NaN is in no bin.

    ``left_profiles`` is read a chunk at a time exactly as in :func:`nearest_chunks`, and a chunk's tables are made resident
    ONCE for both steps: the set the selection ran on is pooled by label where it lies (``kpal_pool_groups_device``, one call
    per chunk, accumulated into R rows on the device).  The chunk is not referenced once the next one is asked for: over
    ``Profile.from_fastq_by_record`` the batches of reads are freed as the scan goes and R tables are kept.  When every chunk
    was in HBM, so are the pools, as rows of one new batch.  Where the fast route of :func:`nearest_chunks` does not apply --
    a user callable, non-integer counts -- the assignment follows its fallbacks and the pooling ``klib.pooled_by``; left
    profiles of different k-mer lengths are a ``ValueError``."""
    from . import klib
    if not (hasattr(right_profiles, '__len__') and hasattr(right_profiles, '__getitem__')):
        right_profiles = list(right_profiles)
    R = len(right_profiles)
    if R < 1:
        raise ValueError('pooled_nearest needs at least one right profile')
    max_bytes = CROSS_MAX_BYTES if max_bytes is None else max_bytes
    indices, distances = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.float64)]
    k = ctx = batch = rows = None      # rows: the R pooled tables on the device (those of `batch`, or an allocation of the call's)
    on_device, started = np.zeros(R, dtype=bool), False
    on_host = {}
    try:
        for chunk, index, value, lset in _nearest_chunks(left_profiles, right_profiles, dist, 1, max_bytes, hand_on=True):
            index, value = index[:, 0], value[:, 0]
            indices.append(index)
            distances.append(value)
            if k is None:
                k = chunk[0].length
            if any(p.length != k for p in chunk):
                raise ValueError('pooled_nearest: profiles of different k-mer lengths')
            labels = np.where(np.isnan(value), -1, index).astype(np.int64)
            if lset is None:
                keys, sums = klib.pooled_by(chunk, [None if r < 0 else r for r in labels.tolist()])
                for r, p in zip(keys, sums):
                    on_host[r] = p.counts if r not in on_host else metrics.mergers['sum'](on_host[r], p.counts)
                continue
            bins = 4 ** k
            if rows is None:
                ctx = lset.ctx
                if all(_device_table(p) is not None for p in chunk):
                    batch = klib._fresh_batch(ctx, R, bins)
                rows = batch.ptr if batch is not None else ctx.alloc(R * 8 * bins)
            ctx.pool_groups_device(len(chunk), bins, lset.ptr, labels, R, rows, accumulate=started)    # (the first call zeroes every row)
            started = True
            on_device |= np.bincount(labels[labels >= 0], minlength=R) > 0
            chunk = lset = None
        pools = [None] * R
        names = {}
        for r in set(np.flatnonzero(on_device).tolist()) | set(on_host):
            names[r] = right_profiles[r].name
        if rows is not None and batch is not None and not on_host:
            for r in names:
                pools[r] = klib.Profile._from_device(batch, r, k, names[r])
        else:
            tables = None
            if rows is not None:
                tables = np.empty((R, 4 ** k), dtype=np.int64)
                ctx.d2h(tables, rows)
            for r in names:
                total = tables[r] if on_device[r] else None
                if r in on_host:
                    total = on_host[r] if total is None else metrics.mergers['sum'](total, on_host[r])
                pools[r] = klib.Profile(total, name=names[r])
    finally:
        if rows is not None and batch is None:
            ctx.sync()
            ctx.free(rows)
    return np.concatenate(indices), np.concatenate(distances), pools


def cross_distance_matrix(left_profiles, right_profiles, output, precision, dist, max_bytes=None):
    """Write the rectangle of :func:`cross_distances` to ``output``: ``Q R``, the Q left names, the R right names, then Q
    lines of R distances, ``precision`` decimals, space separated.  Returns the values."""
    left = list(left_profiles)
    right_names = []

    def named(profiles):
        for p in profiles:
            right_names.append(p.name)
            yield p

    values = cross_distances(left, named(right_profiles), dist, max_bytes=max_bytes)
    print('{0} {1}'.format(len(left), len(right_names)), file=output)
    for name in [p.name for p in left] + right_names:
        print(name, file=output)
    fmt = '{{0:.{0}f}}'.format(precision)
    for row in values:
        output.write(' '.join(fmt.format(v) for v in row))
        output.write('\n')
    return values


def _write_matrix(output, count, values, precision):
    fmt = '{{0:.{0}f}}'.format(precision)
    at = 0
    for i in range(1, count):
        output.write(' '.join(fmt.format(values[at + j]) for j in range(i)))
        output.write('\n')
        at += i


def _device_pair(left, right):
    """(context, device address of left, of right) when both profiles' tables are still in HBM on one context, else None."""
    a, b = _device_table(left), _device_table(right)
    if not a or not b or a[0] is not b[0] or left.length != right.length:
        return None
    return a[0], a[1], b[1]


def _device_matrix(profiles, dist, metric):
    """The matrix values of profiles whose tables are ALL still in HBM (one context, one k) without a transfer: consecutive
    tables of one batch are used where they lie, anything else is gathered by device-to-device copies first.  None when a
    profile has host counts, or when a user-supplied callable keeps the distance in Python."""
    devs = list(map(_device_table, profiles))
    if not devs[0] or not all(d and d[0] is devs[0][0] for d in devs):
        return None
    plain = dist._is_plain() and metric is not None and metric != _native.COSINE
    options = None if plain else dist._native_options()
    if not plain and options is None:
        return None
    ctx, k, P = devs[0][0], profiles[0].length, len(profiles)
    with _DeviceSet(ctx, profiles) as pset:
        if not plain and options.do_smooth:    # one call: a pyramid per profile, the pairs' live elements inside the triangle kernels
            return ctx.smooth_distance_matrix_device(P, k, pset.ptr, options)
        if not plain:    # one call: profiles balanced once, the partner-dependent steps inside the triangle kernels
            return ctx.profile_distance_matrix_device(P, k, pset.ptr, options)
        return ctx.distance_matrix_device(P, k, pset.ptr, metric, do_balance=dist._do_balance)
