"""`WGSassign` command line: drop-in for the hot-path options of the reference's
WGSassign.py (--get_reference_af, --loo, --get_pop_like), running on an AMD MI355X.

Same flags, defaults, stdout lines and output files as the reference (WGSassign.py:24-104,
109-308), including --ne_obs (Fisher information / effective sample sizes) and the two z-score options
(WGSassign.py:311-446).  Options of the reference that are outside this build's scope (mixture
proportions) are recognised and refused with a message.  Installed as the console script `WGSassign` (pyproject.toml; reference
setup.py:48-50).
"""
import argparse
import os
import sys
from datetime import datetime

parser = argparse.ArgumentParser(prog="WGSassign")
parser.add_argument("-b", "--beagle", metavar="FILE",
                    help="Filepath to genotype likelihoods in gzipped Beagle format from ANGSD")
parser.add_argument("-t", "--threads", metavar="INT", type=int, default=1,
                    help="Number of threads (1: chosen automatically). The arithmetic runs on the GPU; the host threads of "
                         "this node's job inflate the Beagle file -- with several ranks the budget is divided between them")
parser.add_argument("-o", "--out", metavar="OUTPUT", default="wgsassign", help="Prefix for output files")
parser.add_argument("--maf_iter", metavar="INT", type=int, default=200,
                    help="Maximum iterations for minor allele frequencies estimation - EM (200)")
parser.add_argument("--maf_tole", metavar="FLOAT", type=float, default=1e-4,
                    help="Tolerance for minor allele frequencies estimation update - EM (1e-4)")
parser.add_argument("--pop_af_IDs", metavar="FILE", help="Filepath to individual IDs and populations for beagle")
parser.add_argument("--get_reference_af", action="store_true",
                    help="Estimate allele frequencies for reference populations")
parser.add_argument("--pop_names", metavar="FILE", help="Filepath to population names of allele frequency file")
parser.add_argument("--loo", action="store_true", help="Perform leave-one-out cross validation")
parser.add_argument("--loo_downsampled_beagle", metavar="FILE",
                    help="Optional Beagle file of downsampled genotype likelihoods to use for LOO assignment.")
parser.add_argument("--pop_af_file", metavar="FILE", help="Filepath to reference population allele frequencies")
parser.add_argument("--get_pop_like", action="store_true",
                    help="Estimate log likelihood of individual assignment to each reference population")
parser.add_argument("--partition_sites", type=int, metavar="INT", default=1,
                    help="Optional: partition sites into INT subsets (by modulo) and report assignment "
                         "log-likelihoods for each subset.")
parser.add_argument("--ne_obs", action="store_true",
                    help="Estimate population and individuals effective sample sizes")
parser.add_argument("--gpus", metavar="INT", type=int, default=1,
                    help="MI355X build: shard the SNPs over INT GPUs of this node, one process per GPU "
                         "(not needed under torchrun or any launcher that sets RANK / WORLD_SIZE)")
parser.add_argument("--get_assignment_z_score", action="store_true", help="Calculate z-score for individuals")
parser.add_argument("--get_reference_z_score", action="store_true", help="Calculate z-score for reference individuals")
parser.add_argument("--ind_ad_file", metavar="FILE",
                    help="Filepath to individual allele depths (text as np.loadtxt reads it, or .npy)")
parser.add_argument("--ind_counts_file", metavar="FILE",
                    help="ANGSD -dumpCounts 4 output (.counts.gz: one header line, A C G T reads per individual); with "
                         "--ind_majmin_file it stands in place of --ind_ad_file")
parser.add_argument("--ind_majmin_file", metavar="FILE",
                    help="Major and minor allele of every site as 0..3 in columns 2 and 3, one header line (the second argument "
                         "of the reference's allele_counts_beagle.py)")
parser.add_argument("--allele_count_threshold", metavar="INT", type=int,
                    help="Minimum number of loci needed to keep a specific allele count combination")
parser.add_argument("--single_read_threshold", action="store_true",
                    help="Use only loci with a single read. Helps reduce computational time since z-score calculation is "
                         "computationally intensive")
parser.add_argument("--ind_start", metavar="INT", type=int, help="Start analysis at this individual index (0-index)")
parser.add_argument("--ind_end", metavar="INT", type=int, help="End analysis at this individual index (0-index)")
# recognised but not provided by this build (out of the hot-path scope)
for _flag in ("--get_em_mix", "--get_mcmc_mix"):
    parser.add_argument(_flag, action="store_true", help=argparse.SUPPRESS)
for _flag in ("--pop_like", "--pop_like_IDs", "--mixture_iter"):
    parser.add_argument(_flag, help=argparse.SUPPRESS)


def windowed_candidate(args, world=1):
    """Whether these options may be scored in site windows (glassy.assignLL_windowed): --get_pop_like alone, on one rank.
    Every other option needs the whole matrix on the device (the EM fit's convergence test couples all sites; the z-scores and
    the leave-one-out re-fits build on it), and a rank of several holds a shard, not a file."""
    others = (args.get_reference_af, args.loo, args.ne_obs, args.get_assignment_z_score, args.get_reference_z_score,
              args.loo_downsampled_beagle)
    return bool(args.get_pop_like) and int(world) == 1 and not any(others)


WINDOWS_ONLY = "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"
SLAB_ALLOC_FAILED = ("hipMalloc of", "for population slab")       # csrc/api.hip: wgs_beagle_create, when the matrix does not fit the device


SET_WINDOW_SITES = ("the matrix was expected to fit the device and does not: set WGSASSIGN_WINDOW_SITES (a multiple of 8192 sites) to "
                    "score the file in site windows")


SET_WINDOW_SITES_Z = ("the matrix was expected to fit the device and does not: set WGSASSIGN_Z_WINDOW_SITES (a multiple of 8192 sites) to "
                      "compute the z-scores in site windows")


SET_WINDOW_SITES_ZREF = ("the matrix was expected to fit the device and does not: set WGSASSIGN_ZREF_WINDOW_SITES (a multiple of 8192 sites) "
                         "to compute the reference z-scores in site windows")


SET_WINDOW_SITES_LOO_DS = ("the two matrices were expected to fit the device and do not: set WGSASSIGN_LOO_DS_WINDOW_SITES (a multiple of 8192 "
                           "sites) to run the leave-one-out on downsampled likelihoods in site windows")


def with_windows_hint(error, candidate=False, z_candidate=False, zref_candidate=False, loo_ds_candidate=False):
    """The error of a resident run whose matrix did not fit the device, saying what windows cover -- or, when the options were
    those windows cover (candidate: the file was only judged to fit; z_candidate: --get_assignment_z_score alone, which has a
    variable of its own; zref_candidate: --get_reference_z_score alone, which has another; loo_ds_candidate: --get_reference_af --loo
    --loo_downsampled_beagle, which has a third), how to ask for them; any other error as it is."""
    if isinstance(error, RuntimeError) and all(part in str(error) for part in SLAB_ALLOC_FAILED):
        return RuntimeError(str(error) + ": " + (SET_WINDOW_SITES_Z if z_candidate else SET_WINDOW_SITES_ZREF if zref_candidate else
                                                 SET_WINDOW_SITES_LOO_DS if loo_ds_candidate else SET_WINDOW_SITES if candidate else
                                                 WINDOWS_ONLY))
    return error


def _window_sites(args, comm, ctx):
    """The window --get_pop_like is scored in, or None for the resident path: WGSASSIGN_WINDOW_SITES when set, else windows only
    when the resident matrix would not fit (windows.plan).  A file whose compressed size alone says that it fits (windows.surely_fits)
    is looked at no further; beyond that the decision costs a cold BGZF file no pass of its own: what its one-pass ingest would
    allocate (the estimate plus a quarter) is tried first."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_candidate(args, comm.world) or not (args.pop_af_file and os.path.isfile(args.pop_af_file)):
        return None                     # (a missing frequency file is reported where it always was)
    try:
        W = windows.env_window_sites()
    except ValueError as e:
        raise SystemExit(str(e))
    if W is not None:
        return W
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        A = np.load(args.pop_af_file, mmap_mode="r")
    except Exception:
        return None                     # (an unreadable frequency file, too, is reported where it always was)
    if A.ndim != 2:
        return None
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        n = st.n
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident(est + est // 4 + 1024, n, A.shape[1], free):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan(m, n, A.shape[1], free)
    except MemoryError as e:
        raise SystemExit(str(e))


def windowed_fit_candidate(args, world=1):
    """Whether these options may be fitted in site windows (emMAF.emMAF_windowed): --get_reference_af alone, on one rank.  With
    --loo or --ne_obs beside it the run has a route of its own (windowed_loo_candidate, windowed_ne_candidate); the z-scores still need
    the whole matrix on the device."""
    others = (args.get_pop_like, args.loo, args.ne_obs, args.get_assignment_z_score, args.get_reference_z_score,
              args.loo_downsampled_beagle)
    return bool(args.get_reference_af) and int(world) == 1 and not any(others)


SET_WINDOW_SITES_FIT = ("the matrix was expected to fit the device and does not: set WGSASSIGN_WINDOW_SITES (a multiple of 8192 sites) to "
                        "fit the file in site windows")


def _fit_window_sites(args, comm, ctx):
    """The window --get_reference_af is fitted in, or None for the resident path: WGSASSIGN_WINDOW_SITES when set, else windows
    only when the resident matrix would not fit (windows.plan_fit), after the same first look as _window_sites takes."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_fit_candidate(args, comm.world) or not (args.pop_af_IDs and os.path.isfile(args.pop_af_IDs)):
        return None                     # (a missing ID file is reported where it always was)
    try:
        W = windows.env_window_sites()
    except ValueError as e:
        raise SystemExit(str(e))
    if W is not None:
        return W
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None                     # (an unreadable ID file, too, is reported where it always was)
    n, K = int(counts.sum()), len(counts)
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident_fit(est + est // 4 + 1024, n, K, free, counts):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_fit(m, n, K, free, counts=counts)
    except MemoryError as e:
        raise SystemExit(str(e))


def windowed_loo_candidate(args, world=1):
    """Whether these options may run in site windows end to end (emMAF.emMAF_windowed, then glassy.loo_windowed):
    --get_reference_af --loo alone, with any --partition_sites, on one rank.  With --ne_obs beside them the run has a route of its own
    (windowed_ne_candidate), and so it has with --loo_downsampled_beagle (two files in lockstep under a site filter:
    windowed_loo_ds_candidate); the z-scores and --get_pop_like beside them still need the whole matrix on the device."""
    others = (args.get_pop_like, args.ne_obs, args.get_assignment_z_score, args.get_reference_z_score, args.loo_downsampled_beagle)
    return bool(args.get_reference_af) and bool(args.loo) and int(world) == 1 and not any(others)


def _loo_window_sites(args, comm, ctx):
    """The window --get_reference_af --loo runs in, or None for the resident path: WGSASSIGN_LOO_WINDOW_SITES when set
    (WGSASSIGN_WINDOW_SITES alone sends no leave-one-out run to windows), else windows only when the resident matrix would not
    fit (windows.plan_loo), after the same first look as _fit_window_sites takes."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_loo_candidate(args, comm.world) or not (args.pop_af_IDs and os.path.isfile(args.pop_af_IDs)):
        return None                     # (a missing ID file is reported where it always was)
    try:
        W = windows.env_window_sites(name=windows.ENV_LOO)
    except ValueError as e:
        raise SystemExit(str(e))
    if W is not None:
        return W
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None                     # (an unreadable ID file, too, is reported where it always was)
    n, K = int(counts.sum()), len(counts)
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident_fit(est + est // 4 + 1024, n, K, free, counts):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_loo(m, n, K, free, counts=counts, P=args.partition_sites)
    except MemoryError as e:
        raise SystemExit(str(e))


def windowed_loo_ds_candidate(args, world=1):
    """Whether these options may run in site windows with a downsampled file scored (emMAF.emMAF_windowed under the reference file's
    site mask, then glassy.loo_windowed with both masks and the second file): --get_reference_af --loo --loo_downsampled_beagle, with any
    --partition_sites, on one rank.  With --ne_obs, --get_pop_like or a z-score option beside them the run stays resident."""
    others = (args.get_pop_like, args.ne_obs, args.get_assignment_z_score, args.get_reference_z_score)
    return bool(args.get_reference_af) and bool(args.loo) and bool(args.loo_downsampled_beagle) and int(world) == 1 and not any(others)


def _loo_ds_window_sites(args, comm, ctx, m_kept=None):
    """The window of KEPT sites --get_reference_af --loo --loo_downsampled_beagle runs in, or None for the resident path:
    WGSASSIGN_LOO_DS_WINDOW_SITES when set (no other variable sends this run to windows), else windows only when the two resident
    matrices would not fit (windows.plan_loo_ds): a pair of files whose compressed sizes together say that they fit
    (windows.surely_fits) is looked at no further.  m_kept: the sites both files keep under their masks, when the caller has them
    (None: the reference file's sites, which bound them)."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_loo_ds_candidate(args, comm.world) or not (args.pop_af_IDs and os.path.isfile(args.pop_af_IDs)):
        return None                     # (a missing ID file is reported where it always was)
    try:
        W = windows.env_window_sites(name=windows.ENV_LOO_DS)
    except ValueError as e:
        raise SystemExit(str(e))
    if W is not None:
        return W
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle) + os.path.getsize(args.loo_downsampled_beagle), free):
        return None
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None                     # (an unreadable ID file, too, is reported where it always was)
    n, K = int(counts.sum()), len(counts)
    if m_kept is None:
        m_kept = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_loo_ds(m_kept, n, K, free, counts=counts, P=args.partition_sites)
    except MemoryError as e:
        raise SystemExit(str(e))


def _run_loo_ds_windowed(args, ctx, W, IDs, pops, sample_names, keep_ref, keep_ds, say):
    """--get_reference_af --loo --loo_downsampled_beagle on files that do not fit (or WGSASSIGN_LOO_DS_WINDOW_SITES), after the names
    passes and the two site masks of the resident run: the fit over the kept sites of the reference file in windows, then the
    leave-one-out run in the same windows with the downsampled file's windows scored beside them; the lines and files of the resident
    run in their order, and one more line on stderr."""
    import numpy as np

    from . import emMAF, glassy, utils
    P = args.partition_sites
    say("Parsing reference population ID file.")
    assert (len(sample_names) == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    af, iters = emMAF.emMAF_windowed(args.beagle, IDs, args.maf_iter, args.maf_tole, W, out=args.out + ".pop_af.npy", ctx=ctx, keep=keep_ref)
    for it in iters:
        if it > 0:
            say("EM (MAF) converged at iteration: " + str(int(it)))
    del af
    say("Saved reference population allele frequencies as " + str(args.out) + ".pop_af.npy (Binary - np.float32)\n")
    say("Column order of populations is: " + str(pops))
    np.savetxt(args.out + ".pop_names.txt", pops, fmt="%s")
    say("Saved reference population names as " + str(args.out) +
        ".pop_names.txt (String: Order of pops for .pop_af.npy, .ne_obs.npy, and fisher_obs.npy files)\n")
    say("Performing leave-one-out cross validation.")
    say(str(len(sample_names)) + " individuals to assign to " + str(len(pops)) + " populations")
    say("Using downsampled GLs for likelihood evaluation in LOO assignment.")
    A = np.load(args.out + ".pop_af.npy", mmap_mode="r")
    ll, parts, loo_iters = glassy.loo_windowed(args.beagle, A, IDs, args.maf_iter, args.maf_tole, W, P, need_parts=P > 1, pop_iters=iters,
                                               ctx=ctx, keep=keep_ref, scored_path=args.loo_downsampled_beagle, scored_keep=keep_ds)
    del A
    stats = glassy.loo_windowed.stats
    for it in loo_iters:
        if it > 0:
            say("EM (MAF) converged at iteration: " + str(int(it)))
    print("wgsassign_amd: leave-one-out on downsampled likelihoods in %d rounds of %d windows of %d kept sites (the downsampled file read "
          "%d time)" % (stats["rounds"], stats["windows"], stats["window_sites"], stats["scored_passes"]), file=sys.stderr, flush=True)
    outfile = f"{args.out}.pop_like_LOO_downsampled.tsv"
    partfile = f"{args.out}.pop_like_LOO_downsampled_partitions_{P}.tsv.gz"
    utils.write_ass_mats(outfile, ll, sample_names, pops, print_part_column=False, sample_locations=IDs[:, 1], doing_LOO=True)
    say(f"Saved leave-one-out cross validation log likelihoods as {outfile}")
    if P > 1:
        utils.write_ass_mats(partfile, parts, sample_names, pops, partition_count=P, print_part_column=True,
                             sample_locations=IDs[:, 1], doing_LOO=True)
        say(f"Saved leave-one-out cross validation log likelihoods from partitioned sites as {partfile}")
    say(f"Column order of populations is: {pops}")


def windowed_ne_candidate(args, world=1):
    """Whether these options may run in site windows end to end with --ne_obs among them (emMAF.emMAF_windowed, then
    fisher.fisher_obs_windowed over the frequencies just written, then glassy.loo_windowed when --loo is given):
    --get_reference_af --ne_obs, with or without --loo and any --partition_sites, on one rank.  The z-scores, --get_pop_like beside
    them and --loo_downsampled_beagle still need the whole matrix on the device."""
    others = (args.get_pop_like, args.get_assignment_z_score, args.get_reference_z_score, args.loo_downsampled_beagle)
    return bool(args.get_reference_af) and bool(args.ne_obs) and int(world) == 1 and not any(others)


def _ne_window_sites(args, comm, ctx):
    """The window --get_reference_af --ne_obs [--loo] runs in, or None for the resident path: WGSASSIGN_NE_WINDOW_SITES when set
    (neither WGSASSIGN_WINDOW_SITES nor WGSASSIGN_LOO_WINDOW_SITES sends an --ne_obs run to windows), else windows only when the
    resident matrix would not fit (windows.plan_ne), after the same first look as _fit_window_sites takes."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_ne_candidate(args, comm.world) or not (args.pop_af_IDs and os.path.isfile(args.pop_af_IDs)):
        return None                     # (a missing ID file is reported where it always was)
    try:
        W = windows.env_window_sites(name=windows.ENV_NE)
    except ValueError as e:
        raise SystemExit(str(e))
    if W is not None:
        return W
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None                     # (an unreadable ID file, too, is reported where it always was)
    n, K = int(counts.sum()), len(counts)
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident_fit(est + est // 4 + 1024, n, K, free, counts):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_ne(m, n, K, free, counts=counts, loo=bool(args.loo), P=args.partition_sites)
    except MemoryError as e:
        raise SystemExit(str(e))


def windowed_z_candidate(args, world=1):
    """Whether these options may run in site windows (zscore.assignment_z_scores_windowed): --get_assignment_z_score alone, on one
    rank.  Its frequencies come from --pop_af_file, so nothing couples the windows but sums that are carried on the device.
    --get_reference_z_score needs masked leave-one-out re-fits whose stopping test runs over the whole file: it has a route of its own
    (windowed_zref_candidate, zscore.reference_z_scores_windowed) and is not this function's; several ranks keep the resident path."""
    others = (args.get_reference_af, args.loo, args.ne_obs, args.get_pop_like, args.get_reference_z_score, args.loo_downsampled_beagle)
    return bool(args.get_assignment_z_score) and int(world) == 1 and not any(others)


def _z_individuals(args, n):
    """How many individuals --ind_start / --ind_end leave of n, for the plan alone (the run checks the range as it always did)."""
    lo = args.ind_start if args.ind_start else 0
    hi = args.ind_end if args.ind_end else n
    return max(1, min(n, hi) - max(0, lo))


def _z_window_sites(args, comm, ctx):
    """(window, individuals per round) --get_assignment_z_score runs in, or None for the resident path: WGSASSIGN_Z_WINDOW_SITES when
    set (no other variable sends the z-scores to windows), else windows only when the resident matrix, depth table and frequencies
    would not fit (windows.plan_z), after the same first look as _window_sites takes."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_z_candidate(args, comm.world) or not (args.pop_af_file and os.path.isfile(args.pop_af_file)):
        return None                     # (a missing frequency file is reported where it always was)
    try:
        forced = windows.env_window_sites(name=windows.ENV_Z)
    except ValueError as e:
        raise SystemExit(str(e))
    if forced is not None:
        return forced, None             # (the rounds of individuals are planned once the file's shape is known)
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        A = np.load(args.pop_af_file, mmap_mode="r")
    except Exception:
        return None                     # (an unreadable frequency file, too, is reported where it always was)
    if A.ndim != 2:
        return None
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        n = st.n
    count = _z_individuals(args, n)
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident_z(est + est // 4 + 1024, n, A.shape[1], count, free):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_z(m, n, A.shape[1], count, free)
    except MemoryError as e:
        raise SystemExit(str(e))


def _run_z_windowed(args, comm, ctx, plan, say, summary):
    """--get_assignment_z_score alone on files that do not fit (or WGSASSIGN_Z_WINDOW_SITES): two passes over the Beagle file and the
    depth file in site windows; the checks, lines and file of the resident run in their order, and one more line on stderr."""
    import numpy as np

    from . import reader_cy, zscore
    W, batch = plan
    index, _, m = reader_cy.ensure_index(args.beagle)
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        n = st.n
    assert os.path.isfile(args.pop_af_IDs), "Population ID file does not exist!!"
    IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
    A = np.load(args.pop_af_file, mmap_mode="r")
    majmin = None
    if args.ind_counts_file:
        majmin = zscore.read_majmin(args.ind_majmin_file)
        if majmin.shape[0] != m:
            raise ValueError("%s has the selectors of %d sites, the Beagle file %d" % (args.ind_majmin_file, majmin.shape[0], m))
    else:
        assert os.path.isfile(args.ind_ad_file), "Individual allele depths file does not exist!"
    assert os.path.isfile(args.pop_names), "Population names file does not exist!!"
    pops = np.loadtxt(args.pop_names, dtype="str")
    assert (n == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    if args.allele_count_threshold is not None:
        assert (args.allele_count_threshold >= 0), "Allele count threshold needs to be greater than/equal to 0!"
    allele_count_threshold = args.allele_count_threshold or 0
    ind_start, ind_end = zscore.ind_range(n, args.ind_start, args.ind_end)
    lines = []
    z_out = zscore.assignment_z_scores_windowed(args.beagle, args.ind_counts_file or args.ind_ad_file, A, IDs, np.atleast_1d(pops),
                                                allele_count_threshold, args.single_read_threshold, ind_start, ind_end, window_sites=W,
                                                say=lines.append, counts=majmin is not None, majmin=majmin, batch=batch, ctx=ctx)
    info, stats = zscore.assignment_z_scores_windowed.info, zscore.assignment_z_scores_windowed.stats
    say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
    summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
    say("Parsing population ID file.")
    say("Parsing population allele frequency file.")
    say("Parsing individual allele depths file.")
    for ln in lines:
        say(ln)
    print("wgsassign_amd: z-scores in %d rounds of 2 passes over %d windows of %d sites (%d bytes downloaded)" %
          (stats["rounds"], stats["windows"], stats["window_sites"], stats["downloaded_bytes"]), file=sys.stderr, flush=True)
    np.savetxt(args.out + ".z_ind.txt", z_out, fmt="%.7f")
    say("Saved " + str(ind_end - ind_start) + " individual z-scores as " + str(args.out) + ".z_ind.txt (text)")


def windowed_zref_candidate(args, world=1):
    """Whether these options may run in site windows (zscore.reference_z_scores_windowed): --get_reference_z_score alone, on one
    rank -- with its ID and name files, the depth options, the thresholds, the individual range, --maf_iter and --maf_tole.  The
    masked leave-one-out fits are carried from window to window like the chain of a SNP shard; several ranks keep the resident path."""
    others = (args.get_reference_af, args.loo, args.ne_obs, args.get_pop_like, args.get_assignment_z_score, args.loo_downsampled_beagle)
    return bool(args.get_reference_z_score) and int(world) == 1 and not any(others)


def _zref_window_sites(args, comm, ctx):
    """(window, individuals per round) --get_reference_z_score runs in, or None for the resident path: WGSASSIGN_ZREF_WINDOW_SITES
    when set (no other variable sends this option to windows), else windows only when the resident matrix, depth table and one batch
    of masked fits would not fit (windows.plan_zref), after the same first look as _z_window_sites takes."""
    import numpy as np

    from . import reader_cy, windows
    if not windowed_zref_candidate(args, comm.world) or not (args.pop_af_IDs and os.path.isfile(args.pop_af_IDs)):
        return None                     # (a missing ID file is reported where it always was)
    try:
        forced = windows.env_window_sites(name=windows.ENV_ZREF)
    except ValueError as e:
        raise SystemExit(str(e))
    if forced is not None:
        return forced, None             # (the rounds of individuals are planned once the file's shape is known)
    free = ctx.mem_info()[0]
    if windows.surely_fits(os.path.getsize(args.beagle), free):
        return None
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None                     # (an unreadable ID file, too, is reported where it always was)
    n, K = int(counts.sum()), len(counts)
    count = _z_individuals(args, n)
    est = None if reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
    if est is not None and windows.fits_resident_zref(est + est // 4 + 1024, n, K, count, free, counts):
        return None
    m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return windows.plan_zref(m, n, K, count, free, args.maf_iter, counts=counts)
    except MemoryError as e:
        raise SystemExit(str(e))


def _run_zref_windowed(args, comm, ctx, plan, IDs, group_of, say, summary):
    """--get_reference_z_score alone on files that do not fit (or WGSASSIGN_ZREF_WINDOW_SITES): passes over the Beagle file and the
    depth file in site windows; the checks, lines and file of the resident run in their order, and one more line on stderr."""
    import numpy as np

    from . import reader_cy, zscore
    W, batch = plan
    index, _, m = reader_cy.ensure_index(args.beagle)
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        n = st.n
    assert os.path.isfile(args.pop_af_IDs), "Population ID file does not exist!!"
    majmin = None
    if args.ind_counts_file:
        majmin = zscore.read_majmin(args.ind_majmin_file)
        if majmin.shape[0] != m:
            raise ValueError("%s has the selectors of %d sites, the Beagle file %d" % (args.ind_majmin_file, majmin.shape[0], m))
    else:
        assert os.path.isfile(args.ind_ad_file), "Individual allele depths file does not exist!"
    assert os.path.isfile(args.pop_names), "Population names file does not exist!!"
    assert (n == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    if args.allele_count_threshold is not None:
        assert (args.allele_count_threshold >= 0), "Allele count threshold needs to be greater than/equal to 0!"
    allele_count_threshold = args.allele_count_threshold or 0
    ind_start, ind_end = zscore.ind_range(n, args.ind_start, args.ind_end)
    lines = []
    z_out = zscore.reference_z_scores_windowed(args.beagle, args.ind_counts_file or args.ind_ad_file, IDs, group_of, args.maf_iter,
                                               args.maf_tole, allele_count_threshold, args.single_read_threshold, ind_start, ind_end,
                                               window_sites=W, say=lines.append, counts=majmin is not None, majmin=majmin, batch=batch,
                                               ctx=ctx)
    info, stats = zscore.reference_z_scores_windowed.info, zscore.reference_z_scores_windowed.stats
    say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
    summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
    say("Parsing population ID file.")
    say("Parsing individual allele depths file.")
    for ln in lines:
        say(ln)
    print("wgsassign_amd: reference z-scores in %d rounds of individuals, %d passes over %d windows of %d sites (%d bytes downloaded)" %
          (stats["rounds"], stats["passes"], stats["windows"], stats["window_sites"], stats["downloaded_bytes"]), file=sys.stderr, flush=True)
    np.savetxt(args.out + ".reference_z_ind.txt", z_out, fmt="%.7f")
    say("Saved " + str(ind_end - ind_start) + " individual z-scores as " + str(args.out) + ".reference_z_ind.txt (text)")


def _run(args, comm):
    """The hot-path options on device-resident data.  Under torchrun (one process per GPU) the SNPs are
    sharded over the ranks: every rank parses and holds only its contiguous SNP range; the EM convergence sums,
    the serial-chain carry and the n x K log-likelihood sums cross ranks through one sum
    all-reduce (RCCL); rank 0 writes the reference's output files."""
    import numpy as np

    from . import emMAF, fisher, glassy, reader_cy, utils
    from .device import AFSet, assign, get_context

    root = comm.rank == 0

    def say(*a):
        if root:
            print(*a)

    ctx = get_context()
    reader_cy.set_threads(args.threads)
    say("Parsing Beagle file.")
    assert os.path.isfile(args.beagle), "Beagle file doesn't exist!"
    IDs = pops = None
    group_of, n_groups = None, 1
    if args.get_reference_af or args.get_reference_z_score:      # one slab per population: the leave-one-out fits sweep their own
        assert os.path.isfile(args.pop_af_IDs), "Reference population ID file does not exist!!"
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        pops = np.unique(IDs[:, 1])
        group_of, n_groups = np.searchsorted(pops, IDs[:, 1]).astype(np.int32), len(pops)

    def summary(samples, m_sites, ends):
        heads = [x for e in ends for x in e[0]]
        tails = [x for e in ends for x in e[1]]
        shown = heads[:m_sites] if m_sites <= 4 else heads[:2] + tails[-2:]
        print(f"sample_names: {len(samples)} samples total: {utils.preview(samples)}")
        print(f"site_names: {m_sites} sites total: " + (", ".join(shown) if m_sites <= 4 else
                                                          ", ".join(shown[:2]) + ", ..., " + ", ".join(shown[2:])))

    W = _window_sites(args, comm, ctx)
    if W is not None:
        # --get_pop_like alone on a file that does not fit (or WGSASSIGN_WINDOW_SITES): scored window by window; the lines of the
        # resident run in their order, and one more on stderr
        A = np.load(args.pop_af_file, mmap_mode="r")
        out = glassy.assignLL_windowed(args.beagle, A, W, ctx=ctx)
        info, stats = glassy.assignLL_windowed.info, glassy.assignLL_windowed.stats
        say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
        summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
        say("Parsing population allele frequency file.")
        say("Calculating likelihood of population assignment")
        say(str(info["n"]) + " individuals to assign to " + str(A.shape[1]) + " populations")
        print("wgsassign_amd: scored in %d windows of %d sites" % (stats["windows"], stats["window_sites"]), file=sys.stderr, flush=True)
        np.savetxt(args.out + ".pop_like.txt", out.astype(np.float32), fmt="%.7f")
        say("Saved population assignment log likelihoods as " + str(args.out) + ".pop_like.txt (text)")
        comm.barrier()
        return

    W = _fit_window_sites(args, comm, ctx)
    W_loo = _loo_window_sites(args, comm, ctx) if W is None else None
    W_ne = _ne_window_sites(args, comm, ctx) if W is None and W_loo is None else None
    if W is not None or W_loo is not None or W_ne is not None:
        # --get_reference_af alone on a file that does not fit (or WGSASSIGN_WINDOW_SITES): fitted window by window in rounds; the
        # lines and files of the resident run, and one more line on stderr.  With --loo beside it (a file that does not fit, or
        # WGSASSIGN_LOO_WINDOW_SITES) the leave-one-out run follows in the same windows, on the frequencies just written.  With
        # --ne_obs (a file that does not fit, or WGSASSIGN_NE_WINDOW_SITES) one pass for the Fisher information comes between them.
        W = W if W is not None else W_loo if W_loo is not None else W_ne
        af, iters = emMAF.emMAF_windowed(args.beagle, IDs, args.maf_iter, args.maf_tole, W, out=args.out + ".pop_af.npy", ctx=ctx)
        info, stats = emMAF.emMAF_windowed.info, emMAF.emMAF_windowed.stats
        say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
        summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
        say("Parsing reference population ID file.")
        for it in iters:
            if it > 0:
                say("EM (MAF) converged at iteration: " + str(int(it)))
        print("wgsassign_amd: fitted in %d rounds of %d windows of %d sites" % (stats["rounds"], stats["windows"], stats["window_sites"]),
              file=sys.stderr, flush=True)
        del af
        say("Saved reference population allele frequencies as " + str(args.out) + ".pop_af.npy (Binary - np.float32)\n")
        say("Column order of populations is: " + str(pops))
        np.savetxt(args.out + ".pop_names.txt", pops, fmt="%s")
        say("Saved reference population names as " + str(args.out) +
            ".pop_names.txt (String: Order of pops for .pop_af.npy, .ne_obs.npy, and fisher_obs.npy files)\n")
        if W_ne is not None:
            say("Estimating Fisher information.")
            A = np.load(args.out + ".pop_af.npy", mmap_mode="r")
            f_obs, ne_obs, ne_obs_mean, ne_ind = fisher.fisher_obs_windowed(args.beagle, A, IDs, W, out=args.out, ctx=ctx)
            del A, f_obs, ne_obs
            stats = fisher.fisher_obs_windowed.stats
            print("wgsassign_amd: Fisher information in %d windows of %d sites" % (stats["windows"], stats["window_sites"]), file=sys.stderr,
                  flush=True)
            say("Saved reference population observed Fisher information per locus as " + str(args.out) +
                ".fisher_obs.npy (Binary - np.float32)\n")
            say("Saved reference population effective sample size estimates per locus as " + str(args.out) +
                ".ne_obs.npy (Binary - np.float32)\n")
            ne_obs_mean_out = np.empty((2, len(pops)), dtype=np.dtype('U25'))
            ne_obs_mean_out[0, :] = pops
            ne_obs_mean_out[1, :] = ne_obs_mean
            np.savetxt(args.out + ".ne_obs.txt", ne_obs_mean_out, fmt="%s")
            say("Saved reference population effective sample size estimates as " + str(args.out) +
                ".ne_obs.txt (String - np.U25)\n")
            say("Estimating individual effective sample sizes.")
            np.savetxt(args.out + ".ne_ind.txt", ne_ind.reshape(-1, 1), fmt="%.7f")
            say("Save individual effective sample sizes as " + str(args.out) + ".ne_ind.txt")
        if W_loo is not None or (W_ne is not None and args.loo):
            P = args.partition_sites
            say("Performing leave-one-out cross validation.")
            say(str(info["n"]) + " individuals to assign to " + str(len(pops)) + " populations")
            A = np.load(args.out + ".pop_af.npy", mmap_mode="r")
            ll, parts, loo_iters = glassy.loo_windowed(args.beagle, A, IDs, args.maf_iter, args.maf_tole, W, P, need_parts=P > 1,
                                                       pop_iters=iters, ctx=ctx)
            del A
            stats = glassy.loo_windowed.stats
            for it in loo_iters:
                if it > 0:
                    say("EM (MAF) converged at iteration: " + str(int(it)))
            print("wgsassign_amd: leave-one-out in %d rounds of %d windows of %d sites" % (stats["rounds"], stats["windows"], stats["window_sites"]),
                  file=sys.stderr, flush=True)
            outfile = f"{args.out}.pop_like_LOO.tsv"
            partfile = f"{args.out}.pop_like_LOO_partitions_{P}.tsv.gz"
            utils.write_ass_mats(outfile, ll, info["sample_names"], pops, print_part_column=False, sample_locations=IDs[:, 1], doing_LOO=True)
            say(f"Saved leave-one-out cross validation log likelihoods as {outfile}")
            if P > 1:
                utils.write_ass_mats(partfile, parts, info["sample_names"], pops, partition_count=P, print_part_column=True,
                                     sample_locations=IDs[:, 1], doing_LOO=True)
                say(f"Saved leave-one-out cross validation log likelihoods from partitioned sites as {partfile}")
            say(f"Column order of populations is: {pops}")
        comm.barrier()
        return

    z_plan = _z_window_sites(args, comm, ctx)
    if z_plan is not None:
        _run_z_windowed(args, comm, ctx, z_plan, say, summary)
        comm.barrier()
        return

    zref_plan = _zref_window_sites(args, comm, ctx)
    if zref_plan is not None:
        _run_zref_windowed(args, comm, ctx, zref_plan, IDs, group_of, say, summary)
        comm.barrier()
        return

    scored = None
    if args.loo_downsampled_beagle:
        # WGSassign.py:172-198 with names-only passes: every rank derives the same two site masks, then
        # parses only its range of the KEPT sites of each file
        assert os.path.isfile(args.loo_downsampled_beagle), "Downsampled beagle file doesn't exist!"
        sample_names, names_ref = reader_cy.read_site_names(args.beagle, comm)
        sample_names_ds, names_ds = reader_cy.read_site_names(args.loo_downsampled_beagle, comm)
        n = len(sample_names)
        say("Loaded " + str(len(names_ref)) + " sites and " + str(n) + " individuals.")
        if root:
            utils.print_sample_and_site_summary(sample_names, names_ref)
        say("Parsing the optional downsampled Beagle file.")
        say("Loaded optional downsampled data set with " + str(len(names_ref)) + " sites and " + str(n) + " individuals.")
        if root:
            utils.print_sample_and_site_summary(sample_names_ds, names_ds)
        if sample_names != sample_names_ds:
            raise ValueError("Sample names in downsampled Beagle file do not match original.")
        say("Retaining only sites from the reference that are in the downsampled beagle file:")
        keep_ref = utils.site_mask(names_ref, names_ds)
        if root and int(np.sum(~keep_ref)) > 0:
            print(f"\tFiltered out {int(np.sum(~keep_ref))} sites not present in the target site list.")
        kept_ref = [x for x, k in zip(names_ref, keep_ref) if k]
        say("Removing sites from downsampled set that were not in the reference (should not occur...):")
        keep_ds = utils.site_mask(names_ds, kept_ref)
        if root and int(np.sum(~keep_ds)) > 0:
            print(f"\tFiltered out {int(np.sum(~keep_ds))} sites not present in the target site list.")
        if kept_ref != [x for x, k in zip(names_ds, keep_ds) if k]:
            raise ValueError("Site names in full and downsampled Beagle do not match after filtering.")
        W_ds = _loo_ds_window_sites(args, comm, ctx, m_kept=len(kept_ref))
        if W_ds is not None:
            # --get_reference_af --loo --loo_downsampled_beagle on files that do not fit (or WGSASSIGN_LOO_DS_WINDOW_SITES): both files
            # in windows of kept sites; the names of both files still live on the host
            del names_ref, names_ds, kept_ref
            _run_loo_ds_windowed(args, ctx, W_ds, IDs, pops, sample_names, keep_ref, keep_ds, say)
            comm.barrier()
            return
        try:
            beagle, _, site_names, m = reader_cy.stream_to_device(args.beagle, group_of, n_groups, ctx=ctx, rank=comm.rank,
                                                                  world=comm.world, keep=keep_ref, comm=comm)
            scored, _, _, _ = reader_cy.stream_to_device(args.loo_downsampled_beagle, group_of, n_groups, ctx=ctx,
                                                         rank=comm.rank, world=comm.world, keep=keep_ds, comm=comm)
        except RuntimeError as e:
            hinted = with_windows_hint(e, loo_ds_candidate=windowed_loo_ds_candidate(args, comm.world))
            if hinted is e:
                raise
            raise hinted from e
    else:
        try:
            beagle, sample_names, site_names, m = reader_cy.stream_to_device(
                args.beagle, group_of, n_groups, ctx=ctx, rank=comm.rank, world=comm.world, comm=comm, names="ends")
        except RuntimeError as e:
            hinted = with_windows_hint(e, windowed_candidate(args, comm.world), windowed_z_candidate(args, comm.world),
                                       zref_candidate=windowed_zref_candidate(args, comm.world))
            if hinted is e:
                raise
            raise hinted from e
        n = beagle.n
        say("Loaded " + str(m) + " sites and " + str(n) + " individuals.")
        ends = comm.allgather_object((site_names[:4], site_names[-4:]))
        if root:
            summary(sample_names, m, ends)

    if args.get_reference_af:
        say("Parsing reference population ID file.")
        assert (n == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
        import contextlib
        import io
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            pops, af, _ = emMAF.emMAF_populations(None, IDs, args.maf_iter, args.maf_tole, beagle=beagle, comm=comm)
        if root:
            sys.stdout.write(buf.getvalue())
        af_full = comm.gather_rows(af)
        if root:
            np.save(args.out + ".pop_af", af_full)
        say("Saved reference population allele frequencies as " + str(args.out) + ".pop_af.npy (Binary - np.float32)\n")
        say("Column order of populations is: " + str(pops))
        if root:
            np.savetxt(args.out + ".pop_names.txt", pops, fmt="%s")
        say("Saved reference population names as " + str(args.out) +
            ".pop_names.txt (String: Order of pops for .pop_af.npy, .ne_obs.npy, and fisher_obs.npy files)\n")
        if args.ne_obs:                      # per-SNP quantities shard trivially; rank 0 assembles and writes
            say("Estimating Fisher information.")
            f_loc, ne_loc = fisher.fisher_obs(None, af, IDs, args.threads, beagle=beagle)
            f_obs, ne_obs = comm.gather_rows(f_loc), comm.gather_rows(ne_loc)
            if root:
                np.save(args.out + ".fisher_obs", f_obs)
            say("Saved reference population observed Fisher information per locus as " + str(args.out) +
                ".fisher_obs.npy (Binary - np.float32)\n")
            if root:
                np.save(args.out + ".ne_obs", ne_obs)
            say("Saved reference population effective sample size estimates per locus as " + str(args.out) +
                ".ne_obs.npy (Binary - np.float32)\n")
            if root:
                ne_obs_mean_out = np.empty((2, len(pops)), dtype=np.dtype('U25'))
                ne_obs_mean_out[0, :] = pops
                ne_obs_mean_out[1, :] = np.mean(ne_obs, axis=0)
                np.savetxt(args.out + ".ne_obs.txt", ne_obs_mean_out, fmt="%s")
            say("Saved reference population effective sample size estimates as " + str(args.out) +
                ".ne_obs.txt (String - np.U25)\n")
            say("Estimating individual effective sample sizes.")
            # np.mean's running float32 total is handed from SNP shard to SNP shard (fisher.fisher_obs_ind)
            ne_ind_full = fisher.fisher_obs_ind(None, af, IDs, args.threads, beagle=beagle, comm=comm, m_total=m)
            if root:
                np.savetxt(args.out + ".ne_ind.txt", ne_ind_full.reshape(-1, 1), fmt="%.7f")
            say("Save individual effective sample sizes as " + str(args.out) + ".ne_ind.txt")

        if args.loo:
            say("Performing leave-one-out cross validation.")
            say(str(n) + " individuals to assign to " + str(len(pops)) + " populations")
            if scored is not None:
                say("Using downsampled GLs for likelihood evaluation in LOO assignment.")
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ll, parts = glassy.loo_device(beagle, scored if scored is not None else beagle, af, group_of,
                                              args.maf_iter, args.maf_tole,
                                              args.partition_sites, comm=comm, need_parts=args.partition_sites > 1)
            if root:
                sys.stdout.write(buf.getvalue())
                suffix = "_downsampled" if scored is not None else ""
                outfile = f"{args.out}.pop_like_LOO{suffix}.tsv"
                partfile = f"{args.out}.pop_like_LOO{suffix}_partitions_{args.partition_sites}.tsv.gz"
                utils.write_ass_mats(outfile, ll, sample_names, pops, print_part_column=False,
                                     sample_locations=IDs[:, 1], doing_LOO=True)
                print(f"Saved leave-one-out cross validation log likelihoods as {outfile}")
                if args.partition_sites > 1:
                    utils.write_ass_mats(partfile, parts, sample_names, pops, partition_count=args.partition_sites,
                                         print_part_column=True, sample_locations=IDs[:, 1], doing_LOO=True)
                    print(f"Saved leave-one-out cross validation log likelihoods from partitioned sites as {partfile}")
                print(f"Column order of populations is: {pops}")

    if args.get_pop_like:
        say("Parsing population allele frequency file.")
        assert os.path.isfile(args.pop_af_file), "Population allele frequency file does not exist!!"
        from .comm import shard_range
        lo, hi = shard_range(m, comm.rank, comm.world)
        A = np.ascontiguousarray(np.load(args.pop_af_file, mmap_mode="r")[lo:hi], dtype=np.float32)
        say("Calculating likelihood of population assignment")
        say(str(n) + " individuals to assign to " + str(A.shape[1]) + " populations")
        afs = AFSet.from_host(A, ctx=ctx)
        out, _ = assign(beagle, afs, comm=comm)
        afs.close()
        if root:
            np.savetxt(args.out + ".pop_like.txt", out.astype(np.float32), fmt="%.7f")
        say("Saved population assignment log likelihoods as " + str(args.out) + ".pop_like.txt (text)")
    for flavour in ("reference", "assignment"):
        if getattr(args, "get_%s_z_score" % flavour):
            _z_scores(args, flavour, beagle, group_of, m, n, say, root, comm)
    if scored is not None:
        scored.close()
    beagle.close()
    comm.barrier()


def _z_scores(args, flavour, beagle, group_of, m, n, say, root, comm):
    """WGSassign.py:311-393 (reference) / 395-446 (assignment): same files read, same checks and texts, same output.  Several
    ranks: each takes the rows of its SNP shard from the frequency, depth and selector files (m: the sites of all shards); rank 0
    receives the z-scores and writes the file."""
    import numpy as np

    from . import zscore
    from .comm import shard_range
    from .device import AFSet
    lo, hi = shard_range(m, comm.rank, comm.world)
    say("Parsing population ID file.")
    assert os.path.isfile(args.pop_af_IDs), "Population ID file does not exist!!"
    IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
    afs = None
    if flavour == "assignment":
        say("Parsing population allele frequency file.")
        assert os.path.isfile(args.pop_af_file), "Population allele frequency file does not exist!!"
        A = np.load(args.pop_af_file, mmap_mode="r")
    say("Parsing individual allele depths file.")
    majmin = None
    if args.ind_counts_file:
        majmin = zscore.read_majmin(args.ind_majmin_file)       # (checked once before the Beagle file was opened: depth_options)
        if comm.world > 1:
            if majmin.shape[0] != m:
                raise ValueError("%s has the selectors of %d sites, the Beagle file %d" % (args.ind_majmin_file, majmin.shape[0], m))
            majmin = np.ascontiguousarray(majmin[lo:hi])
    else:
        assert os.path.isfile(args.ind_ad_file), "Individual allele depths file does not exist!"
    assert os.path.isfile(args.pop_names), "Population names file does not exist!!"
    pops = np.loadtxt(args.pop_names, dtype="str")
    assert (n == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    if args.allele_count_threshold is not None:
        assert (args.allele_count_threshold >= 0), "Allele count threshold needs to be greater than/equal to 0!"
        allele_count_threshold = args.allele_count_threshold
    else:
        allele_count_threshold = 0
    ind_start, ind_end = zscore.ind_range(n, args.ind_start, args.ind_end)
    # streamed and tokenised on the device: no m x 2n array on the host (csrc/ingest.hip: depth_tokenise_kernel)
    if comm.world > 1:
        depth = zscore.DepthTable.from_file(beagle, args.ind_counts_file or args.ind_ad_file, counts=majmin is not None, majmin=majmin,
                                            first_row=lo, m_total=m)
    else:
        depth = zscore.DepthTable.from_file(beagle, args.ind_counts_file or args.ind_ad_file, counts=majmin is not None, majmin=majmin)
    shards = comm if comm.world > 1 else None
    if flavour == "assignment":
        if A.shape[0] != m:
            raise ValueError("the allele frequency file has %d sites, the Beagle file %d" % (A.shape[0], m))
        afs = AFSet.from_host(np.ascontiguousarray(A[lo:hi], dtype=np.float32), ctx=beagle.ctx)
        z_out = zscore.assignment_z_scores(beagle, depth, IDs, np.atleast_1d(pops), afs, allele_count_threshold,
                                           args.single_read_threshold, ind_start, ind_end, say=say, comm=shards)
        afs.close()
        name = ".z_ind.txt"
    else:
        z_out = zscore.reference_z_scores(beagle, depth, IDs, group_of, args.maf_iter, args.maf_tole, allele_count_threshold,
                                          args.single_read_threshold, ind_start, ind_end, say=say, comm=shards)
        name = ".reference_z_ind.txt"
    depth.close()
    if root:
        np.savetxt(args.out + name, z_out, fmt="%.7f")
    say("Saved " + str(ind_end - ind_start) + " individual z-scores as " + str(args.out) + name + " (text)")


def depth_options(args):
    """--ind_counts_file / --ind_majmin_file against --ind_ad_file, before any large file is opened."""
    if args.ind_counts_file and args.ind_ad_file:
        raise SystemExit("--ind_counts_file (with --ind_majmin_file) stands in place of --ind_ad_file: give one of the two")
    if bool(args.ind_counts_file) != bool(args.ind_majmin_file):
        raise SystemExit("--ind_counts_file and --ind_majmin_file go together: %s is missing" %
                         ("--ind_majmin_file" if args.ind_counts_file else "--ind_counts_file"))
    if args.ind_counts_file:
        for path, what in ((args.ind_counts_file, "ANGSD counts"), (args.ind_majmin_file, "major/minor allele")):
            if not os.path.isfile(path):
                raise SystemExit("%s file %s does not exist" % (what, path))
        from . import zscore
        try:
            zscore.read_majmin(args.ind_majmin_file)
        except ValueError as e:
            raise SystemExit(str(e))


def main(argv=None):
    args = parser.parse_args(argv)
    if len(sys.argv) < 2 and argv is None:
        parser.print_help()
        sys.exit()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU, started here before anything touches the device; they come back through this function
        # with RANK / WORLD_SIZE set
        from .comm import launch_local_ranks
        sys.exit(launch_local_ranks(args.gpus, [sys.executable, "-m", "wgsassign_amd.WGSassign"] +
                                    list(sys.argv[1:] if argv is None else argv)))
    from .comm import init_from_env
    comm = init_from_env()          # LocalComm for one process; one rank per GPU under --gpus N / torchrun
    root = comm.rank == 0
    if root:
        print("WGSassign")
        print("Matt DeSaix.")
        print("Using " + str(args.threads) + " thread(s).\n")

    if args.loo_downsampled_beagle and not args.loo:
        raise ValueError("The --loo_downsampled_beagle option requires that --loo is also specified.")
    for unsupported in ("get_em_mix", "get_mcmc_mix"):
        if getattr(args, unsupported):
            raise SystemExit("--%s is outside the scope of the MI355X build (EM allele frequencies, Fisher "
                             "information, leave-one-out and assignment likelihoods only)" % unsupported)
    if args.get_assignment_z_score or args.get_reference_z_score:
        depth_options(args)
        if comm.world > 1 and getattr(comm, "handle", None) is None:
            # the class sums and the masked chain cross the SNP shards inside the library: before any file is opened
            raise SystemExit("--get_assignment_z_score / --get_reference_z_score over several ranks need the library's own communicator "
                             "(WGSASSIGN_COMM=rccl or socket); %s has none" % type(comm).__name__)

    if root:        # log-file of non-default arguments (WGSassign.py:127-141)
        full, deaf = vars(args), vars(parser.parse_args([]))
        with open(args.out + ".args", "w") as fh:
            fh.write("WGSassign\n")
            fh.write("Time: " + datetime.now().strftime("%d/%m/%Y %H:%M:%S") + "\n")
            fh.write("Directory: " + str(os.getcwd()) + "\n")
            fh.write("Options:\n")
            for key in full:
                if full[key] != deaf[key]:
                    if type(full[key]) is bool:
                        fh.write("\t-" + str(key) + "\n")
                    else:
                        fh.write("\t-" + str(key) + " " + str(full[key]) + "\n")

    if args.beagle is None:
        return
    # One code path for one or many GPUs: the Beagle file is streamed chunk by chunk into the device
    # slabs (host memory stays at one chunk; the reference holds two full copies of the matrix).
    from .comm import COMM_DIVERGED, CollectiveMismatch
    try:
        return _run(args, comm)
    except CollectiveMismatch as e:
        # the ranks issued different collectives: nothing computed from here on could be trusted, and nothing is retried --
        # every rank that sees it leaves with its own message; the launcher ends the others and reports this status
        print("wgsassign_amd: rank %d: %s" % (comm.rank, e), file=sys.stderr, flush=True)
        sys.stderr.flush()
        os._exit(COMM_DIVERGED)         # (not sys.exit: a peer blocked inside a collective would keep atexit handlers waiting)


if __name__ == "__main__":
    main()
