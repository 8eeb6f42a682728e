"""Drop-in for ``kpal.kmer``: the seventeen command functions (kpal/kmer.py:52-700) and the command line
``main`` (kpal/kmer.py:703-975; ``python -m kpal_amd ...``).  They are orchestration: handles in, profiles
through :mod:`kpal_amd.klib` / :mod:`kpal_amd.kdistlib` (HIP kernels), text or an HDF5 handle out.  Same
sub-commands, arguments, defaults, output lines and ``ValueError`` messages as the reference.

Profile files are whatever the caller opens -- an ``h5py.File`` in kPAL; this module only uses the
handle operations kPAL itself uses (``handle['profiles']``, ``handle['profiles/<name>'][:]``,
``create_dataset``, ``attrs``, ``flush``).
"""
from __future__ import print_function

import importlib
import os
import re

import argparse
import sys

import numpy as np

from . import files, kdistlib, klib, metrics
from .files import FileType, ProfileFileType, doc_split

LENGTH_ERROR = 'k-mer lengths of the files differ'
NAMES_COUNT_ERROR = 'number of profile names does not match number of profiles'
PAIRED_NAMES_COUNT_ERROR = 'number of left and right profile names do not match'
PREFIX_COUNT_ERROR = 'number of name prefixes does not match number of profiles'
POOL_NEEDS_NEAREST = '--pool needs --nearest'

# dotted path of an importable function, e.g. ``package.module.function`` (kpal/kmer.py:36-38)
_DOTTED_PATH = re.compile(r'[_a-zA-Z][_a-zA-Z0-9]*(\.[_a-zA-Z][_a-zA-Z0-9]*)+$')


def _name_from_handle(handle):
    """File name without directory and extension, or None for nameless handles and the
    ``<stdin>``-like ones (kpal/kmer.py:41-48)."""
    name = getattr(handle, 'name', None)
    if name is None or str(name).startswith('<'):
        return None
    return os.path.splitext(os.path.basename(str(name)))[0]


def _custom_function(definition, arguments):
    """A user-supplied function given on the command line: either a dotted import path or a Python
    expression over ``arguments`` with NumPy available as ``np`` (kpal/kmer.py:173-181,577-599).
    Such a callable never enters a kernel; klib / kdistlib run it through NumPy as the reference does."""
    if _DOTTED_PATH.match(definition):
        module, attribute = definition.rsplit('.', 1)
        return getattr(importlib.import_module(module), attribute)
    return eval('lambda %s: %s' % (arguments, definition), {'np': np})


def _profile_names(handle, names):
    return names or sorted(handle['profiles'])


def _fixed(precision, value):
    return '{{0:.{0}f}}'.format(precision).format(value)


def convert(input_handles, output_handle, names=None):
    """Save k-mer profiles from files in the old plaintext format (kPAL < 1.0.0) to a k-mer profile file in
    the current HDF5 format.

    (kpal/kmer.py:52-74.)  Profiles are named by ``names``, else after the input files, else numbered."""
    names = names or [_name_from_handle(handle) for handle in input_handles]
    if len(names) != len(input_handles):
        raise ValueError(NAMES_COUNT_ERROR)
    for handle, name in zip(input_handles, names):
        klib.Profile.from_file_old_format(handle, name=name).save(output_handle)


def cat(input_handles, output_handle, names=None, prefixes=None):
    """Save k-mer profiles from several files to one k-mer profile file.

    (kpal/kmer.py:77-109.)  A name that a file does not hold is skipped for that file -- it may have been
    given to select from another one; ``prefixes`` (one per file) keep equal names apart."""
    prefixes = prefixes or ['' for _ in input_handles]
    if len(prefixes) != len(input_handles):
        raise ValueError(PREFIX_COUNT_ERROR)
    for handle, prefix in zip(input_handles, prefixes):
        for name in names or sorted(handle['profiles']):
            try:
                profile = klib.Profile.from_file(handle, name=name)
            except KeyError:
                continue
            profile.save(output_handle, name=prefix + name)


def count(input_handles, output_handle, size, names=None, by_record=False, fastq=False, min_quality=None, phred64=False,
          by_window=None, step=None, by_read=False):
    """k-mer profiles of FASTA files (kpal/kmer.py:112-146): one profile per file, or per record
    with ``by_record`` (record names, prefixed by the file's name when several files are given).
    With ``fastq`` the inputs are four-line FASTQ files, one profile per file (beyond the reference); ``min_quality`` masks
    bases of a lower Phred quality, read with offset 64 instead of 33 under ``phred64``.
    With ``by_window`` = W (beyond the reference) there is one profile per sliding window of W bases of every record, ``step``
    bases apart (default W; it must divide W), named ``<record>:<start>-<end>`` and prefixed like the records' profiles.
    With ``by_read`` (beyond the reference) the inputs are four-line FASTQ files and there is one profile per read, named and
    prefixed as ``by_record`` names records; with ``by_window`` as well, one per sliding window of every read.  ``fastq`` next
    to it is redundant."""
    if by_read and by_record:
        raise ValueError('--by-read and --by-record exclude each other (--by-read is the --by-record of FASTQ input)')
    if fastq and by_record:
        raise ValueError('--by-record does not apply to FASTQ input (one profile per read is --by-read)')
    if by_window is not None and by_record:
        raise ValueError('--by-window and --by-record exclude each other (a window profile is named after its record already)')
    if by_window is not None and fastq and not by_read:
        raise ValueError('--by-window does not apply to FASTQ input (windows of reads are --by-read --by-window)')
    if step is not None and by_window is None:
        raise ValueError('--step applies to --by-window only')
    if by_window is not None:
        klib._window_arguments(size, by_window, step)
    if not (fastq or by_read) and (min_quality is not None or phred64):
        raise ValueError('--min-quality and --phred64 apply to FASTQ input only (add --fastq or --by-read)')
    if by_read:
        klib._read_arguments(size, min_quality, 64 if phred64 else 33)
    names = names or [_name_from_handle(handle) for handle in input_handles]
    if len(names) != len(input_handles):
        raise ValueError(NAMES_COUNT_ERROR)
    several = len(input_handles) > 1
    for handle, name in zip(input_handles, names):
        if by_read and by_window is not None:
            profiles = klib.Profile.from_fastq_by_window(handle, size, by_window, step=step, prefix=name if several else None,
                                                         min_quality=min_quality, quality_offset=64 if phred64 else 33)
        elif by_read:
            profiles = klib.Profile.from_fastq_by_record(handle, size, prefix=name if several else None, min_quality=min_quality,
                                                         quality_offset=64 if phred64 else 33)
        elif fastq:
            profiles = [klib.Profile.from_fastq(handle, size, name=name, min_quality=min_quality,
                                                quality_offset=64 if phred64 else 33)]
        elif by_record:
            profiles = klib.Profile.from_fasta_by_record(handle, size, prefix=name if several else None)
        elif by_window is not None:
            profiles = klib.Profile.from_fasta_by_window(handle, size, by_window, step=step, prefix=name if several else None)
        else:
            profiles = [klib.Profile.from_fasta(handle, size, name=name)]
        for profile in profiles:
            profile.save(output_handle)


def merge(input_handle_left, input_handle_right, output_handle, names_left=None, names_right=None, merger='sum',
          custom_merger=None):
    """Pairwise merge of the profiles of two files, linked by position in the (sorted) name lists
    (kpal/kmer.py:149-201); the result is named after both inputs."""
    names_left = _profile_names(input_handle_left, names_left)
    names_right = _profile_names(input_handle_right, names_right)
    if len(names_left) != len(names_right):
        raise ValueError(PAIRED_NAMES_COUNT_ERROR)
    function = _custom_function(custom_merger, 'left, right') if custom_merger else metrics.mergers[merger]
    for name_left, name_right in zip(names_left, names_right):
        left = klib.Profile.from_file(input_handle_left, name=name_left)
        right = klib.Profile.from_file(input_handle_right, name=name_right)
        if left.length != right.length:
            raise ValueError(LENGTH_ERROR)
        right.merge(left, function)      # merger(right, left), as the reference calls it
        right.save(output_handle, name=name_left if name_left == name_right else name_left + '_' + name_right)


def balance(input_handle, output_handle, names=None):
    """Balanced copies of the profiles of a file (kpal/kmer.py:203-219), a group of profiles balanced by one launch."""
    for group in _profile_groups(input_handle, _profile_names(input_handle, names)):
        klib.balance_profiles(group)
        for profile in group:
            profile.save(output_handle)


def _profile_groups(input_handle, names):
    """The profiles ``names`` of a file, read in groups of at most ``klib._RECORD_BATCH_BYTES`` of counts (never less than one
    profile): what the set functions of klib take at a time."""
    group, size = [], 0
    for name in names:
        profile = klib.Profile.from_file(input_handle, name=name)
        group.append(profile)
        size += np.asanyarray(profile.counts).nbytes
        if size >= klib._RECORD_BATCH_BYTES:
            yield group
            group, size = [], 0
    if group:
        yield group


def get_balance(input_handle, output_handle, precision=10, names=None):
    """``name balance`` lines: the multiset distance between the forward and the
    reverse-complement half of each profile (kpal/kmer.py:222-247) -- one fused kernel over all profiles of a group."""
    for group in _profile_groups(input_handle, _profile_names(input_handle, names)):
        for profile, score in zip(group, klib.strand_balances(group, 'prod')):
            print(profile.name, _fixed(precision, score), file=output_handle)


def get_stats(input_handle, output_handle, precision=10, names=None):
    """``name mean std`` lines (kpal/kmer.py:250-271), the summaries of a group of profiles from one set call."""
    for group in _profile_groups(input_handle, _profile_names(input_handle, names)):
        for profile, stats in zip(group, klib.summaries(group)):
            print(profile.name, _fixed(precision, stats['mean']), _fixed(precision, stats['std']), file=output_handle)


def distribution(input_handle, output_handle, names=None):
    """Calculate the distribution of the values in k-mer profiles: ``name count number-of-k-mers`` lines.

    (kpal/kmer.py:274-295.)  The spectra of a group of profiles come from one set call on the device."""
    for group in _profile_groups(input_handle, _profile_names(input_handle, names)):
        for profile, pairs in zip(group, klib.distributions(group)):
            print('\n'.join('{0} {1} {2}'.format(profile.name, value, number) for value, number in pairs), file=output_handle)


def info(input_handle, output_handle, names=None):
    """Print some information about k-mer profiles.

    (kpal/kmer.py:298-335.)  The five summaries of the profiles of a group come from one set call on the device."""
    names = _profile_names(input_handle, names)

    def text(value):
        return value.decode('utf-8', 'replace') if isinstance(value, bytes) else value

    print('File format version:', text(input_handle.attrs['version']), file=output_handle)
    print('Produced by:', text(input_handle.attrs['producer']), file=output_handle)
    for group in _profile_groups(input_handle, names):
        for profile, stats in zip(group, klib.summaries(group)):
            print('', file=output_handle)
            print('Profile:', profile.name, file=output_handle)
            print('- k-mer length:', str(profile.length), '({0} k-mers)'.format(profile.number), file=output_handle)
            print('- Zero counts:', str(profile.number - stats['non_zero']), file=output_handle)
            print('- Non-zero counts:', str(stats['non_zero']), file=output_handle)
            print('- Sum of counts:', str(stats['total']), file=output_handle)
            print('- Mean of counts:', '{0:.3f}'.format(stats['mean']), file=output_handle)
            print('- Median of counts:', '{0:.3f}'.format(stats['median']), file=output_handle)
            print('- Standard deviation of counts:', '{0:.3f}'.format(stats['std']), file=output_handle)


def get_count(input_handle, output_handle, word, names=None):
    """Retrieve the counts in k-mer profiles for a particular word.

    (kpal/kmer.py:338-362.)"""
    for name in _profile_names(input_handle, names):
        profile = klib.Profile.from_file(input_handle, name=name)
        if profile.length != len(word):
            raise ValueError('the length of the query does not match the profile length')
        try:
            offset = profile.dna_to_binary(word)
        except KeyError:
            raise ValueError('the input is not a valid DNA sequence')
        print(name, str(profile.counts[offset]), file=output_handle)


class _LengthMismatch(ValueError):
    """LENGTH_ERROR for a linked pair: the one error of ``_paired`` behind which the earlier pairs are still written."""


def _paired(input_handle_left, input_handle_right, names_left, names_right):
    """The (left, right) profile pairs of the two-file commands, linked by position in the name lists.  Unequal numbers of
    names raise here, at the call -- before a caller evaluates a custom function, like the reference; the pairs are read as
    the generator that is returned goes."""
    names_left = _profile_names(input_handle_left, names_left)
    names_right = _profile_names(input_handle_right, names_right)
    if len(names_left) != len(names_right):
        raise ValueError(PAIRED_NAMES_COUNT_ERROR)

    def pairs():
        for name_left, name_right in zip(names_left, names_right):
            left = klib.Profile.from_file(input_handle_left, name=name_left)
            right = klib.Profile.from_file(input_handle_right, name=name_right)
            if left.length != right.length:
                raise _LengthMismatch(LENGTH_ERROR)
            yield left, right

    return pairs()


def _paired_groups(input_handle_left, input_handle_right, names_left, names_right):
    """The pairs of ``_paired`` as ``(lefts, rights)`` lists of at most ``klib._RECORD_BATCH_BYTES`` of counts over both sides
    (never less than one pair), sized as ``_profile_groups`` sizes its groups: what the set functions of linked pairs take at
    a time.  A pair of two k-mer lengths ends the groups with LENGTH_ERROR AFTER the pairs before it have been handed out, so
    that they are written as the pair-by-pair loop wrote them; any other error is raised at once."""
    pairs = _paired(input_handle_left, input_handle_right, names_left, names_right)

    def groups():
        lefts, rights, size, mismatch = [], [], 0, None
        try:
            for left, right in pairs:
                lefts.append(left)
                rights.append(right)
                size += np.asanyarray(left.counts).nbytes + np.asanyarray(right.counts).nbytes
                if size >= klib._RECORD_BATCH_BYTES:
                    yield lefts, rights
                    lefts, rights, size = [], [], 0
        except _LengthMismatch as error:
            mismatch = error
        if lefts:
            yield lefts, rights
        if mismatch is not None:
            raise mismatch

    return groups()


def positive(input_handle_left, input_handle_right, output_handle_left, output_handle_right, names_left=None,
             names_right=None):
    """Only keep counts that are positive in both k-mer profiles; several profiles per file are linked by
    name and processed pairwise.

    (kpal/kmer.py:365-401.)"""
    for left, right in _paired(input_handle_left, input_handle_right, names_left, names_right):
        left.counts = metrics.positive(left.counts, right.counts)
        right.counts = metrics.positive(right.counts, left.counts)
        left.save(output_handle_left)
        right.save(output_handle_right)


def scale(input_handle_left, input_handle_right, output_handle_left, output_handle_right, names_left=None,
          names_right=None, down=False):
    """Scale two profiles such that the total number of k-mers is equal; several profiles per file are
    linked by name and processed pairwise.

    (kpal/kmer.py:404-444.)  The scaled counts are floats; ``save`` stores them as int64 like the reference."""
    for left, right in _paired(input_handle_left, input_handle_right, names_left, names_right):
        scale_left, scale_right = metrics.get_scale(left.counts, right.counts)
        if down:
            scale_left, scale_right = metrics.scale_down(scale_left, scale_right)
        left.counts = left.counts * scale_left
        right.counts = right.counts * scale_right
        left.save(output_handle_left)
        right.save(output_handle_right)


def shrink(input_handle, output_handle, factor, names=None):
    """Shrink k-mer profiles, effectively reducing k.

    (kpal/kmer.py:447-464.)  A group of profiles is shrunk by one launch."""
    for group in _profile_groups(input_handle, _profile_names(input_handle, names)):
        klib.shrink_profiles(group, factor)
        for profile in group:
            profile.save(output_handle)


def shuffle(input_handle, output_handle, names=None):
    """Randomise k-mer profiles.

    (kpal/kmer.py:467-483.)"""
    for name in _profile_names(input_handle, names):
        profile = klib.Profile.from_file(input_handle, name=name)
        profile.shuffle()
        profile.save(output_handle)


def smooth(input_handle_left, input_handle_right, output_handle_left, output_handle_right, names_left=None,
           names_right=None, summary='min', custom_summary=None, threshold=0):
    """Smooth two profiles by collapsing sub-profiles; several profiles per file are linked by name and
    processed pairwise.

    (kpal/kmer.py:486-538.)  Both files are read in groups of at most ``klib._RECORD_BATCH_BYTES`` of counts over both sides; a
    group is smoothed by one set call on the device (``klib.smooth_profiles``)."""
    groups = _paired_groups(input_handle_left, input_handle_right, names_left, names_right)
    function = _custom_function(custom_summary, 'values') if custom_summary else metrics.summary[summary]
    dist = kdistlib.ProfileDistance(summary=function, threshold=threshold)
    for lefts, rights in groups:
        klib.smooth_profiles(lefts, rights, dist)
        for left, right in zip(lefts, rights):
            left.save(output_handle_left)
            right.save(output_handle_right)


def _profile_distance(distance_function, pairwise, custom_pairwise, do_smooth, summary, custom_summary, threshold,
                      do_scale, down, do_positive, do_balance):
    summary_function = _custom_function(custom_summary, 'values') if custom_summary else metrics.summary[summary]
    pairwise_function = (_custom_function(custom_pairwise, 'left, right') if custom_pairwise
                         else metrics.pairwise[pairwise])
    return kdistlib.ProfileDistance(do_balance=do_balance, do_positive=do_positive, do_smooth=do_smooth,
                                    summary=summary_function, threshold=threshold, do_scale=do_scale, down=down,
                                    pairwise=pairwise_function,
                                    distance_function=metrics.vector_distance[distance_function])


def distance(input_handle_left, input_handle_right, output_handle, names_left=None, names_right=None,
             distance_function='default', pairwise='prod', custom_pairwise=None, do_smooth=False, summary='min',
             custom_summary=None, threshold=0, do_scale=False, down=False, do_positive=False, do_balance=False,
             precision=10):
    """``left right distance`` lines for the profiles of two files, linked pairwise
    (kpal/kmer.py:541-620).  Both files are read in groups of at most ``klib._RECORD_BATCH_BYTES`` of counts over both sides;
    a group's distances come from one set call on the device."""
    groups = _paired_groups(input_handle_left, input_handle_right, names_left, names_right)
    dist = _profile_distance(distance_function, pairwise, custom_pairwise, do_smooth, summary, custom_summary,
                             threshold, do_scale, down, do_positive, do_balance)
    for lefts, rights in groups:
        # a group of pairs is one set call (kdistlib.paired_distances); the lines are those of the loop over dist.distance
        for left, right, value in zip(lefts, rights, kdistlib.paired_distances(lefts, rights, dist)):
            print(left.name, right.name, _fixed(precision, value), file=output_handle)


def distance_matrix(input_handle, output_handle, names=None, distance_function='default', pairwise='prod',
                    custom_pairwise=None, do_smooth=False, summary='min', custom_summary=None, threshold=0,
                    do_scale=False, down=False, do_positive=False, do_balance=False, precision=10):
    """Lower-triangular distance matrix of the profiles of a file (kpal/kmer.py:623-700); all pairs
    in one kernel launch for the built-in functions."""
    names = _profile_names(input_handle, names)
    if len(names) < 2:
        raise ValueError('you must give at least two k-mer profiles')
    dist = _profile_distance(distance_function, pairwise, custom_pairwise, do_smooth, summary, custom_summary,
                             threshold, do_scale, down, do_positive, do_balance)
    profiles = []
    for name in names:
        profiles.append(klib.Profile.from_file(input_handle, name=name))
        if profiles[0].length != profiles[-1].length:
            raise ValueError(LENGTH_ERROR)
    kdistlib.distance_matrix(profiles, output_handle, precision, dist)


def cross(input_handle_left, input_handle_right, output_handle, names_left=None, names_right=None,
          distance_function='default', pairwise='prod', custom_pairwise=None, do_smooth=False, summary='min',
          custom_summary=None, threshold=0, do_scale=False, down=False, do_positive=False, do_balance=False,
          precision=10, nearest=None, pool=None):
    """Distances of every profile of the left file to every profile of the right file: ``Q R``, the left names, the
    right names, then Q lines of R distances; with --nearest N, ``left right distance`` lines of the N closest right
    profiles per left profile instead; with --pool FILE next to it, FILE receives for every right profile that is the
    closest of some left profile the pooled (summed) profile of those left profiles, under the right profile's name.

    A fixed number of kernel launches per chunk of the right file for the built-in functions; the right file is read profile by
    profile, so only a chunk of it is resident at a time."""
    names_left = _profile_names(input_handle_left, names_left)
    names_right = _profile_names(input_handle_right, names_right)
    if not names_left or not names_right:
        raise ValueError('you must give at least one k-mer profile on each side')
    if nearest is not None and nearest < 1:
        raise ValueError('--nearest needs a positive number')
    if pool is not None and nearest is None:
        raise ValueError(POOL_NEEDS_NEAREST)
    dist = _profile_distance(distance_function, pairwise, custom_pairwise, do_smooth, summary, custom_summary,
                             threshold, do_scale, down, do_positive, do_balance)
    if nearest is not None:
        _cross_nearest(input_handle_left, names_left, input_handle_right, names_right, output_handle, dist, precision, nearest, pool)
        return
    left = [klib.Profile.from_file(input_handle_left, name=name) for name in names_left]

    def right():
        for name in names_right:
            profile = klib.Profile.from_file(input_handle_right, name=name)
            if profile.length != left[0].length:
                raise ValueError(LENGTH_ERROR)
            yield profile

    if any(profile.length != left[0].length for profile in left):
        raise ValueError(LENGTH_ERROR)
    kdistlib.cross_distance_matrix(left, right(), output_handle, precision, dist)


class _FileProfiles(object):
    """The profiles ``names`` of an open k-mer file as a sequence that reads a profile when it is asked for it; ``lengths``:
    a one-element list the first profile read puts its k-mer length in -- a profile of another length is LENGTH_ERROR."""

    def __init__(self, handle, names, lengths):
        self.handle, self.names, self.lengths = handle, names, lengths

    def __len__(self):
        return len(self.names)

    def _read(self, name):
        profile = klib.Profile.from_file(self.handle, name=name)
        if not self.lengths:
            self.lengths.append(profile.length)
        if profile.length != self.lengths[0]:
            raise ValueError(LENGTH_ERROR)
        return profile

    def __getitem__(self, item):
        if isinstance(item, slice):
            return [self._read(name) for name in self.names[item]]
        return self._read(self.names[item])


def _cross_nearest(input_handle_left, names_left, input_handle_right, names_right, output_handle, dist, precision, nearest, pool=None):
    """``left right distance`` lines of the ``nearest`` closest right profiles of every left profile.  The left file is read in
    groups (``_profile_groups``) and the right file chunk by chunk when it does not fit the device at once; the distances are
    selected on the device (``kdistlib.nearest_chunks``), so no Q x R rectangle is built.  ``pool``: an open profile file that
    receives one profile per right name that is the closest (the first hit; a NaN distance is no hit) of a left profile -- the
    sum of those left profiles, pooled group of the left file by group of the left file (``klib.pooled_by``) -- in the order
    of the right names."""
    lengths = []

    def left():
        for group in _profile_groups(input_handle_left, names_left):
            for profile in group:
                if not lengths:
                    lengths.append(profile.length)
                if profile.length != lengths[0]:
                    raise ValueError(LENGTH_ERROR)
                yield profile

    right = _FileProfiles(input_handle_right, names_right, lengths)
    pools = {}
    for chunk, indices, distances in kdistlib.nearest_chunks(left(), right, dist, nearest):
        for profile, row, values in zip(chunk, indices, distances):
            for r, value in zip(row, values):
                print(profile.name, names_right[r], _fixed(precision, value), file=output_handle)
        if pool is not None:
            hits = [None if np.isnan(d) else int(r) for r, d in zip(indices[:, 0], distances[:, 0])]
            for r, pooled in zip(*klib.pooled_by(chunk, hits)):
                pools[r] = pooled if r not in pools else klib.pooled([pools[r], pooled])
    for r in sorted(pools):
        pools[r].save(pool, name=names_right[r])


def _parsers():
    """The option groups shared by the sub-commands (kpal/kmer.py:712-824), as argparse parents."""
    def parent():
        return argparse.ArgumentParser(add_help=False)

    p = {}
    p['multi_input'] = parent()
    p['multi_input'].add_argument('input_handles', metavar='INPUT', type=FileType('r'), nargs='*', default=[sys.stdin],
                                  help='input file (default: stdin)')
    p['input_profile'] = parent()
    p['input_profile'].add_argument('input_handle', metavar='INPUT', type=ProfileFileType('r'), help='input k-mer profile file')
    p['input_profile'].add_argument('-p', '--profiles', dest='names', metavar='NAME', type=str, nargs='+',
                                    help='names of the k-mer profiles to consider (default: all profiles in INPUT, in '
                                    'alphabetical order)')
    p['multi_input_profile'] = parent()
    p['multi_input_profile'].add_argument('input_handles', metavar='INPUT', type=ProfileFileType('r'), nargs='+',
                                          help='input k-mer profile file')
    p['multi_input_profile'].add_argument('-p', '--profiles', dest='names', metavar='NAME', type=str, nargs='+',
                                          help='names of the k-mer profiles to consider (default: all profiles per INPUT, '
                                          'in alphabetical order)')
    p['paired_input_profile'] = parent()
    p['paired_input_profile'].add_argument('input_handle_left', metavar='INPUT_LEFT', type=ProfileFileType('r'),
                                           help='input k-mer profile file (left)')
    p['paired_input_profile'].add_argument('input_handle_right', metavar='INPUT_RIGHT', type=ProfileFileType('r'),
                                           help='input k-mer profile file (right)')
    p['paired_input_profile'].add_argument('-l', '--profiles-left', dest='names_left', metavar='NAME', type=str, nargs='+',
                                           help='names of the k-mer profiles to consider (left) (default: all profiles '
                                           'in INPUT_LEFT, in alphabetical order)')
    p['paired_input_profile'].add_argument('-r', '--profiles-right', dest='names_right', metavar='NAME', type=str, nargs='+',
                                           help='names of the k-mer profiles to consider (right) (default: all profiles '
                                           'in INPUT_RIGHT, in alphabetical order)')
    p['output'] = parent()
    p['output'].add_argument('output_handle', metavar='OUTPUT', type=FileType('w'), help='output file')
    p['output_profile'] = parent()
    p['output_profile'].add_argument('output_handle', metavar='OUTPUT', type=ProfileFileType('w'),
                                     help='output k-mer profile file')
    p['paired_output_profile'] = parent()
    p['paired_output_profile'].add_argument('output_handle_left', metavar='OUTPUT_LEFT', type=ProfileFileType('w'),
                                            help='output k-mer profile file (left)')
    p['paired_output_profile'].add_argument('output_handle_right', metavar='OUTPUT_RIGHT', type=ProfileFileType('w'),
                                            help='output k-mer profile file (right)')
    p['scale'] = parent()
    p['scale'].add_argument('-d', dest='down', action='store_true', help='scale down')
    p['smooth'] = parent()
    p['smooth'].add_argument('-s', dest='summary', type=str, default='min', choices=metrics.summary,
                             help='summary function for dynamic smoothing (default: %(default)s)')
    p['smooth'].add_argument('-M', '--custom-summary', metavar='STRING', type=str, dest='custom_summary',
                             help='custom Python summary function, specified either by an expression over the NumPy '
                             'ndarray "values" (e.g., "np.max(values)"), or an importable name (e.g., '
                             '"package.module.summary") that can be called with an ndarray as argument')
    p['smooth'].add_argument('-t', dest='threshold', metavar='INT', type=int, default=0,
                             help='threshold for the summary function (default: %(default)s)')
    p['precision'] = parent()
    p['precision'].add_argument('-n', metavar='INT', dest='precision', type=int, default=10,
                                help='precision in number of decimals (default: %(default)s)')
    p['dist'] = argparse.ArgumentParser(add_help=False, parents=[p['scale'], p['smooth'], p['precision']])
    p['dist'].add_argument('-b', '--balance', dest='do_balance', action='store_true', help='balance the profiles')
    p['dist'].add_argument('--positive', dest='do_positive', action='store_true', help='use only positive values')
    p['dist'].add_argument('-S', '--scale', dest='do_scale', action='store_true', help='scale the profiles')
    p['dist'].add_argument('-m', '--smooth', dest='do_smooth', action='store_true', help='smooth the profiles')
    p['dist'].add_argument('-D', dest='distance_function', type=str, default='default', choices=metrics.vector_distance,
                           help='choose distance function (default: %(default)s)')
    p['dist'].add_argument('-P', dest='pairwise', type=str, default='prod', choices=metrics.pairwise,
                           help='paiwise distance function for the multiset distance (default: %(default)s)')
    p['dist'].add_argument('-f', '--pairwise-function', metavar='STRING', dest='custom_pairwise', type=str,
                           help='custom Python pairwise function, specified either by an expression over the two NumPy '
                           'ndarrays "left" and "right" (e.g., "abs(left - right) / (left + right + 1)"), or an importable '
                           'name (e.g., "package.module.pairwise") that can be called with two ndarrays as arguments')
    return p


def build_parser():
    """The ``kpal`` command line (kpal/kmer.py:826-964): seventeen sub-commands, same options and defaults, and ``cross``."""
    p = _parsers()
    parser = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter, description=files.USAGE[0],
                                     epilog=files.USAGE[1])
    parser.add_argument('-v', action='version', version=files.version(parser.prog))
    subparsers = parser.add_subparsers(dest='subcommand')
    subparsers.required = True

    def command(name, func, parents, **defaults):
        sub = subparsers.add_parser(name, parents=[p[key] for key in parents], description=doc_split(func))
        sub.set_defaults(func=func, **defaults)
        return sub

    sub = command('convert', convert, ['multi_input', 'output_profile'])
    sub.add_argument('-p', '--profiles', dest='names', metavar='NAME', type=str, nargs='+',
                     help='names for the saved k-mer profiles, one per INPUT (default: profiles are named according to '
                     'the input filenames, or numbered consecutively from 1 if no filenames are available)')
    sub = command('cat', cat, ['multi_input_profile', 'output_profile'])
    sub.add_argument('-x', '--prefixes', dest='prefixes', metavar='PREFIX', type=str, nargs='+',
                     help='prefixes to use for the saved k-mer profile names, one per INPUT (default: profile names are '
                     'assumed to be disjoint and no prefix is used)')
    sub = command('count', count, ['multi_input', 'output_profile'])
    sub.add_argument('-p', '--profiles', dest='names', metavar='NAME', type=str, nargs='+',
                     help='names for the created k-mer profiles, one per INPUT (default: profiles are named according to '
                     'the input filenames, or numbered consecutively from 1 if no filenames are available)')
    sub.add_argument('-k', dest='size', metavar='SIZE', type=int, default=9, help='k-mer size (%(type)s default: %(default)s)')
    sub.add_argument('--by-record', '-r', dest='by_record', action='store_true',
                     help='make a k-mer profile per FASTA record instead of a k-mer profile per FASTA file (profiles are '
                     'named by the record names and prefixed according to --profiles if more than one INPUT is given)')
    sub.add_argument('--by-window', dest='by_window', metavar='W', type=int, default=None,
                     help='make a k-mer profile per sliding window of W bases of every FASTA record (profiles are named '
                     'RECORD:START-END, 1-based and inclusive, and prefixed like those of --by-record)')
    sub.add_argument('--step', dest='step', metavar='S', type=int, default=None,
                     help='with --by-window: bases between the starts of two windows (a divisor of W; default: W)')
    sub.add_argument('--fastq', dest='fastq', action='store_true',
                     help='the INPUTs are four-line FASTQ files of reads (one k-mer profile per file)')
    sub.add_argument('--by-read', dest='by_read', action='store_true',
                     help='the INPUTs are four-line FASTQ files: make a k-mer profile per read (profiles are named by the '
                     'read names and prefixed like those of --by-record); with --by-window W, per sliding window of every read')
    sub.add_argument('--min-quality', dest='min_quality', metavar='Q', type=int, default=None,
                     help='with --fastq or --by-read: mask bases whose Phred quality is below Q (0..93; default: no mask)')
    sub.add_argument('--phred64', dest='phred64', action='store_true',
                     help='with --fastq or --by-read: quality bytes are Phred + 64 (default: Phred + 33)')
    sub = command('merge', merge, ['paired_input_profile', 'output_profile'])
    sub.add_argument('-m', dest='merger', type=str, default='sum', choices=metrics.mergers,
                     help='merge function (default: %(default)s)')
    sub.add_argument('-c', '--custom-merger', dest='custom_merger', metavar='STRING', type=str,
                     help='custom Python merge function, specified either by an expression over the two NumPy ndarrays '
                     '"left" and "right" (e.g., "np.add(left, right)"), or an importable name (e.g., '
                     '"package.module.merge") that can be called with two ndarrays as arguments')
    command('balance', balance, ['input_profile', 'output_profile'])
    command('showbalance', get_balance, ['input_profile', 'precision'], output_handle=sys.stdout)
    command('stats', get_stats, ['input_profile', 'precision'], output_handle=sys.stdout)
    command('distr', distribution, ['input_profile', 'output'])
    command('info', info, ['input_profile'], output_handle=sys.stdout)
    sub = command('getcount', get_count, ['input_profile'], output_handle=sys.stdout)
    sub.add_argument('word', metavar='WORD', type=str, help='the word in question')
    command('positive', positive, ['paired_input_profile', 'paired_output_profile'])
    command('scale', scale, ['paired_input_profile', 'paired_output_profile', 'scale'])
    sub = command('shrink', shrink, ['input_profile', 'output_profile'])
    sub.add_argument('-f', '--factor', dest='factor', metavar='INT', type=int, default=1,
                     help='shrinking factor (default: %(default)s)')
    command('shuffle', shuffle, ['input_profile', 'output_profile'])
    command('smooth', smooth, ['paired_input_profile', 'paired_output_profile', 'smooth'])
    command('distance', distance, ['paired_input_profile', 'dist'], output_handle=sys.stdout)
    command('matrix', distance_matrix, ['input_profile', 'output', 'dist'])
    sub = command('cross', cross, ['paired_input_profile', 'output', 'dist'])
    sub.add_argument('--nearest', dest='nearest', metavar='N', type=int, default=None,
                     help='write "left right distance" lines for the N closest right profiles of every left profile '
                     'instead of the matrix')
    sub.add_argument('--pool', dest='pool', metavar='FILE', type=ProfileFileType('w'), default=None,
                     help='with --nearest: write to the k-mer profile file FILE, for every right profile that is the closest '
                     'of some left profile, the pooled (summed) profile of those left profiles under the right profile\'s name')
    parse_cross = sub.parse_known_args

    def parse_cross_checked(args=None, namespace=None, sub=sub):
        namespace, rest = parse_cross(args, namespace)
        if namespace.pool is not None and namespace.nearest is None:
            sub.error(POOL_NEEDS_NEAREST)
        return namespace, rest

    sub.parse_known_args = parse_cross_checked     # (the two options are checked against each other where they are parsed)
    return parser


def main(args=None):
    """Command line interface (kpal/kmer.py:703-975): ``args`` defaults to ``sys.argv[1:]``; a ``ValueError``
    of a command and an unreadable / existing file end in the parser's usage error (exit status 2)."""
    parser = build_parser()
    try:
        arguments = parser.parse_args(args)
    except IOError as error:
        parser.error(error)
    keywords = dict((key, value) for key, value in vars(arguments).items() if key not in ('func', 'subcommand'))
    try:
        arguments.func(**keywords)
    except ValueError as error:
        parser.error(error)
