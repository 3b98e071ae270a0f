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

from . import windows

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



# ---- the windowed routes: one table, one selector -------------------------------------------------------------

# the options that decide the route; every other argument (--partition_sites, the files, the thresholds) goes with any of them
OPTION_FLAGS = ("get_reference_af", "loo", "ne_obs", "get_pop_like", "get_assignment_z_score", "get_reference_z_score",
                "loo_downsampled_beagle")

WINDOWS_ONLY = "windowed scoring (WGSASSIGN_WINDOW_SITES) covers --get_pop_like on one rank only"
SLAB_ALLOC_FAILED = ("hipMalloc of", "for population slab")       # csrc/api.hip: wgs_beagle_create, when the matrix does not fit the device
SET_WINDOW_SITES = ("the matrix was expected to fit the device and does not: set WGSASSIGN_WINDOW_SITES (a multiple of 8192 sites) to "
                    "score the file in site windows")
SET_WINDOW_SITES_FIT = ("the matrix was expected to fit the device and does not: set WGSASSIGN_WINDOW_SITES (a multiple of 8192 sites) to "
                        "fit the file in site windows")
SET_WINDOW_SITES_Z = ("the matrix was expected to fit the device and does not: set WGSASSIGN_Z_WINDOW_SITES (a multiple of 8192 sites) to "
                      "compute the z-scores in site windows")
SET_WINDOW_SITES_ZREF = ("the matrix was expected to fit the device and does not: set WGSASSIGN_ZREF_WINDOW_SITES (a multiple of 8192 sites) "
                         "to compute the reference z-scores in site windows")
SET_WINDOW_SITES_LOO_DS = ("the two matrices were expected to fit the device and do not: set WGSASSIGN_LOO_DS_WINDOW_SITES (a multiple of 8192 "
                           "sites) to run the leave-one-out on downsampled likelihoods in site windows")


def _shape_from_frequencies(args):
    """(n, K, None) from --pop_af_file (K) and the Beagle header (n); None when the frequency file cannot tell (an unreadable one
    is reported where it always was)."""
    import numpy as np

    from . import reader_cy
    try:
        A = np.load(args.pop_af_file, mmap_mode="r")
    except Exception:
        return None
    if A.ndim != 2:
        return None
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        return st.n, A.shape[1], None


def _shape_from_ids(args):
    """(n, K, counts) from --pop_af_IDs; None when the file cannot tell (an unreadable one is reported where it always was)."""
    import numpy as np
    try:
        IDs = np.loadtxt(args.pop_af_IDs, delimiter="\t", dtype="str")
        counts = np.unique(IDs[:, 1], return_counts=True)[1]
    except Exception:
        return None
    return int(counts.sum()), len(counts), counts


class _Route:
    """One windowed route of the command line.  requires / allows: the OPTION_FLAGS it needs and those that may stand beside them (any
    other sends the run to the resident path); env: its variable; shape: the input file that tells n, K and the populations' sizes,
    and how; fits(m, n, K, counts, count, free): its resident-fit test for the estimated sites of a file without a cached index (None:
    the sites are counted outright); plan(m, n, K, counts, count, free, args): its planner; hint: what with_windows_hint says of it;
    sizes: the files whose compressed sizes windows.surely_fits looks at; rounds: the plan is (window, individuals per round) and
    count the individuals --ind_start / --ind_end leave."""

    def __init__(self, requires, allows, env, shape, fits, plan, hint=None, sizes=("beagle",), rounds=False):
        self.requires, self.allows, self.env, self.fits, self.plan, self.hint = requires, allows, env, fits, plan, hint
        self.shape_file, self.shape = shape
        self.sizes, self.rounds = sizes, rounds

    def candidate(self, args, world):
        """All required options, one rank, and no option but the required and the allowed."""
        beside = [flag for flag in OPTION_FLAGS if flag not in self.requires + self.allows]
        return all(bool(getattr(args, flag)) for flag in self.requires) and int(world) == 1 and not any(getattr(args, flag) for flag in beside)


_FREQUENCIES, _IDS = ("pop_af_file", _shape_from_frequencies), ("pop_af_IDs", _shape_from_ids)


def _fits_fit(m, n, K, counts, count, free):
    return windows.fits_resident_fit(m, n, K, free, counts)


ROUTES = {
    "score": _Route(("get_pop_like",), (), windows.ENV, _FREQUENCIES, hint=SET_WINDOW_SITES,
                    fits=lambda m, n, K, counts, count, free: windows.fits_resident(m, n, K, free),
                    plan=lambda m, n, K, counts, count, free, args: windows.plan(m, n, K, free)),
    "fit": _Route(("get_reference_af",), (), windows.ENV, _IDS, hint=SET_WINDOW_SITES_FIT, fits=_fits_fit,
                  plan=lambda m, n, K, counts, count, free, args: windows.plan_fit(m, n, K, free, counts=counts)),
    "loo": _Route(("get_reference_af", "loo"), (), windows.ENV_LOO, _IDS, fits=_fits_fit,
                  plan=lambda m, n, K, counts, count, free, args: windows.plan_loo(m, n, K, free, counts=counts, P=args.partition_sites)),
    "loo_ds": _Route(("get_reference_af", "loo", "loo_downsampled_beagle"), (), windows.ENV_LOO_DS, _IDS, hint=SET_WINDOW_SITES_LOO_DS,
                     fits=None, sizes=("beagle", "loo_downsampled_beagle"),
                     plan=lambda m, n, K, counts, count, free, args: windows.plan_loo_ds(m, n, K, free, counts=counts, P=args.partition_sites)),
    "ne": _Route(("get_reference_af", "ne_obs"), ("loo",), windows.ENV_NE, _IDS, fits=_fits_fit,
                 plan=lambda m, n, K, counts, count, free, args: windows.plan_ne(m, n, K, free, counts=counts, loo=bool(args.loo),
                                                                                  P=args.partition_sites)),
    "z": _Route(("get_assignment_z_score",), (), windows.ENV_Z, _FREQUENCIES, hint=SET_WINDOW_SITES_Z, rounds=True,
                fits=lambda m, n, K, counts, count, free: windows.fits_resident_z(m, n, K, count, free),
                plan=lambda m, n, K, counts, count, free, args: windows.plan_z(m, n, K, count, free)),
    "zref": _Route(("get_reference_z_score",), (), windows.ENV_ZREF, _IDS, hint=SET_WINDOW_SITES_ZREF, rounds=True,
                   fits=lambda m, n, K, counts, count, free: windows.fits_resident_zref(m, n, K, count, free, counts),
                   plan=lambda m, n, K, counts, count, free, args: windows.plan_zref(m, n, K, count, free, args.maf_iter, counts=counts)),
}


def _z_individuals(args, n):
    """How many individuals --ind_start / --ind_end leave of n, for the plan alone (the run checks the range as it always did)."""
    lo = args.ind_start if args.ind_start else 0
    hi = args.ind_end if args.ind_end else n
    return max(1, min(n, hi) - max(0, lo))


def _route_window_sites(route, args, comm, ctx, m=None):
    """The window a route's options run in -- (window, individuals per round) for a route with rounds --, or None for the resident
    path: the route's variable when it is set (no other variable sends the run to windows; the device is asked nothing, and the
    rounds are planned once the file's shape is known), else windows only when the resident objects would not fit (the route's
    planner).  A file whose compressed size alone says that it fits (windows.surely_fits) is looked at no further; beyond that the
    decision costs a cold BGZF file no pass of its own: what its one-pass ingest would allocate (the estimate plus a quarter) is tried
    first.  m: the sites, when the caller has them.  A missing or unreadable input file is left to the resident path, which reports
    it where it always did."""
    from . import reader_cy
    shape_file = getattr(args, route.shape_file)
    if not route.candidate(args, comm.world) or not (shape_file and os.path.isfile(shape_file)):
        return None
    try:
        forced = windows.env_window_sites(name=route.env)
    except ValueError as e:
        raise SystemExit(str(e))
    if forced is not None:
        return (forced, None) if route.rounds else forced
    free = ctx.mem_info()[0]
    if windows.surely_fits(sum(os.path.getsize(getattr(args, file)) for file in route.sizes), free):
        return None
    shape = route.shape(args)
    if shape is None:
        return None
    n, K, counts = shape
    count = _z_individuals(args, n) if route.rounds else None
    if m is None:
        est = None if route.fits is None or reader_cy._index_is_cached(args.beagle) else reader_cy.estimate_sites(args.beagle)
        if est is not None and route.fits(est + est // 4 + 1024, n, K, counts, count, free):
            return None
        m = reader_cy.ensure_index(args.beagle)[2]
    try:
        return route.plan(m, n, K, counts, count, free, args)
    except MemoryError as e:
        raise SystemExit(str(e))


def windowed_candidate(args, world=1):
    """Whether these options may be scored in site windows (glassy.assignLL_windowed): --get_pop_like alone, on one rank.  (A rank
    of several holds a shard, not a file.)"""
    return ROUTES["score"].candidate(args, world)


def windowed_fit_candidate(args, world=1):
    """Whether these options may be fitted in site windows (emMAF.emMAF_windowed): --get_reference_af alone, on one rank."""
    return ROUTES["fit"].candidate(args, world)


def windowed_loo_candidate(args, world=1):
    """Whether these options may run in site windows end to end (emMAF.emMAF_windowed, then glassy.loo_windowed):
    --get_reference_af --loo alone, with any --partition_sites, on one rank."""
    return ROUTES["loo"].candidate(args, world)


def windowed_loo_ds_candidate(args, world=1):
    """... with a downsampled file scored (both files in lockstep under their site masks): --get_reference_af --loo
    --loo_downsampled_beagle, with any --partition_sites, on one rank."""
    return ROUTES["loo_ds"].candidate(args, world)


def windowed_ne_candidate(args, world=1):
    """... with --ne_obs among them (fisher.fisher_obs_windowed between the fit and the leave-one-out run): --get_reference_af
    --ne_obs, with or without --loo and any --partition_sites, on one rank."""
    return ROUTES["ne"].candidate(args, world)


def windowed_z_candidate(args, world=1):
    """Whether these options may run in site windows (zscore.assignment_z_scores_windowed): --get_assignment_z_score alone, on one
    rank."""
    return ROUTES["z"].candidate(args, world)


def windowed_zref_candidate(args, world=1):
    """Whether these options may run in site windows (zscore.reference_z_scores_windowed): --get_reference_z_score alone, on one
    rank."""
    return ROUTES["zref"].candidate(args, world)


def _window_sites(args, comm, ctx):
    """The window --get_pop_like is scored in, or None for the resident path (_route_window_sites)."""
    return _route_window_sites(ROUTES["score"], args, comm, ctx)


def _fit_window_sites(args, comm, ctx):
    """The window --get_reference_af is fitted in, or None."""
    return _route_window_sites(ROUTES["fit"], args, comm, ctx)


def _loo_window_sites(args, comm, ctx):
    """The window --get_reference_af --loo runs in, or None."""
    return _route_window_sites(ROUTES["loo"], args, comm, ctx)


def _loo_ds_window_sites(args, comm, ctx, m_kept=None):
    """The window of KEPT sites --get_reference_af --loo --loo_downsampled_beagle runs in, or None.  m_kept: the sites both files keep
    under their masks, when the caller has them (None: the reference file's sites, which bound them)."""
    return _route_window_sites(ROUTES["loo_ds"], args, comm, ctx, m_kept)


def _ne_window_sites(args, comm, ctx):
    """The window --get_reference_af --ne_obs [--loo] runs in, or None."""
    return _route_window_sites(ROUTES["ne"], args, comm, ctx)


def _z_window_sites(args, comm, ctx):
    """(window, individuals per round) --get_assignment_z_score runs in, or None."""
    return _route_window_sites(ROUTES["z"], args, comm, ctx)


def _zref_window_sites(args, comm, ctx):
    """(window, individuals per round) --get_reference_z_score runs in, or None."""
    return _route_window_sites(ROUTES["zref"], args, comm, ctx)


def with_windows_hint(error, candidate=False, z_candidate=False, zref_candidate=False, loo_ds_candidate=False):
    """The error of a resident run whose matrix did not fit the device, saying what windows cover -- or, when the options were
    those of a route (candidate: --get_pop_like alone, whose file was only judged to fit; z_candidate, zref_candidate,
    loo_ds_candidate: the routes with a variable of their own), how to ask for them; any other error as it is."""
    if isinstance(error, RuntimeError) and all(part in str(error) for part in SLAB_ALLOC_FAILED):
        asked = [name for name, given in (("z", z_candidate), ("zref", zref_candidate), ("loo_ds", loo_ds_candidate), ("score", candidate))
                 if given]
        return RuntimeError(str(error) + ": " + (ROUTES[asked[0]].hint if asked else WINDOWS_ONLY))
    return error


def _raise_hinted(error, args, world):
    """Raise with_windows_hint's error for these options in place of a slab allocation that failed; any other error as it came."""
    hinted = with_windows_hint(error, *(ROUTES[name].candidate(args, world) for name in ("score", "z", "zref", "loo_ds")))
    if hinted is error:
        raise error
    raise hinted from error


# ---- output blocks that the resident and the windowed runs share ----------------------------------------------------------------------

def _say_converged(iters, say):
    for it in iters:
        if it > 0:
            say("EM (MAF) converged at iteration: " + str(int(it)))


def _save_names(args, pops, say, root=True):
    """The lines of the frequency file (written by the caller) and the population names file with its line."""
    import numpy as np
    say("Saved reference population allele frequencies as " + str(args.out) + ".pop_af.npy (Binary - np.float32)\n")
    say("Column order of populations is: " + str(pops))
    if root:
        np.savetxt(args.out + ".pop_names.txt", pops, fmt="%s")
    say("Saved reference population names as " + str(args.out) +
        ".pop_names.txt (String: Order of pops for .pop_af.npy, .ne_obs.npy, and fisher_obs.npy files)\n")


def _save_ne_obs(args, pops, say, ne_obs_mean, ne_ind, per_locus=None, root=True):
    """The --ne_obs files and lines.  per_locus: (f_obs, ne_obs) still to be saved (None: the windowed pass has written them);
    ne_obs_mean: np.mean(ne_obs, axis=0), on the root; ne_ind: called for the individuals' sizes on every rank once their line is out."""
    import numpy as np
    if root and per_locus is not None:
        np.save(args.out + ".fisher_obs", per_locus[0])
    say("Saved reference population observed Fisher information per locus as " + str(args.out) +
        ".fisher_obs.npy (Binary - np.float32)\n")
    if root and per_locus is not None:
        np.save(args.out + ".ne_obs", per_locus[1])
    say("Saved reference population effective sample size estimates per locus as " + str(args.out) +
        ".ne_obs.npy (Binary - np.float32)\n")
    if root:
        ne_obs_mean_out = np.empty((2, len(pops)), dtype=np.dtype('U25'))
        ne_obs_mean_out[0, :] = pops
        ne_obs_mean_out[1, :] = ne_obs_mean
        np.savetxt(args.out + ".ne_obs.txt", ne_obs_mean_out, fmt="%s")
    say("Saved reference population effective sample size estimates as " + str(args.out) +
        ".ne_obs.txt (String - np.U25)\n")
    say("Estimating individual effective sample sizes.")
    ne_ind = ne_ind()
    if root:
        np.savetxt(args.out + ".ne_ind.txt", ne_ind.reshape(-1, 1), fmt="%.7f")
    say("Save individual effective sample sizes as " + str(args.out) + ".ne_ind.txt")


def _save_loo(args, ll, parts, sample_names, pops, IDs, say, suffix=""):
    """The leave-one-out files and lines (on the root): the totals, and the partition sums when there are several partitions."""
    from . import utils
    P = args.partition_sites
    outfile = f"{args.out}.pop_like_LOO{suffix}.tsv"
    partfile = f"{args.out}.pop_like_LOO{suffix}_partitions_{P}.tsv.gz"
    utils.write_ass_mats(outfile, ll, sample_names, pops, print_part_column=False, sample_locations=IDs[:, 1], doing_LOO=True)
    say(f"Saved leave-one-out cross validation log likelihoods as {outfile}")
    if P > 1:
        utils.write_ass_mats(partfile, parts, sample_names, pops, partition_count=P, print_part_column=True,
                             sample_locations=IDs[:, 1], doing_LOO=True)
        say(f"Saved leave-one-out cross validation log likelihoods from partitioned sites as {partfile}")
    say(f"Column order of populations is: {pops}")


# ---- the windowed runs: the lines and files of the resident run in their order, and one more line per pass on stderr -------------------

def _run_score_windowed(args, ctx, W, say, summary):
    """--get_pop_like alone on a file that does not fit (or WGSASSIGN_WINDOW_SITES): scored window by window."""
    import numpy as np

    from . import glassy
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


def _loo_windowed(args, ctx, W, IDs, pops, sample_names, pop_iters, say, keep_ref=None, keep_ds=None):
    """The leave-one-out run in the windows of the fit, on the frequencies it has just written; with --loo_downsampled_beagle the
    downsampled file's windows are scored beside them (keep_ref, keep_ds: the two site masks)."""
    import numpy as np

    from . import glassy
    P, scored = args.partition_sites, args.loo_downsampled_beagle
    say("Performing leave-one-out cross validation.")
    say(str(len(sample_names)) + " individuals to assign to " + str(len(pops)) + " populations")
    if scored:
        say("Using downsampled GLs for likelihood evaluation in LOO assignment.")
    A = np.load(args.out + ".pop_af.npy", mmap_mode="r")
    ll, parts, loo_iters = glassy.loo_windowed(args.beagle, A, IDs, args.maf_iter, args.maf_tole, W, P, need_parts=P > 1, pop_iters=pop_iters,
                                               ctx=ctx, keep=keep_ref, scored_path=scored, scored_keep=keep_ds)
    del A
    stats = glassy.loo_windowed.stats
    _say_converged(loo_iters, say)
    if scored:
        print("wgsassign_amd: leave-one-out on downsampled likelihoods in %d rounds of %d windows of %d kept sites (the downsampled file "
              "read %d time)" % (stats["rounds"], stats["windows"], stats["window_sites"], stats["scored_passes"]), file=sys.stderr, flush=True)
    else:
        print("wgsassign_amd: leave-one-out in %d rounds of %d windows of %d sites" % (stats["rounds"], stats["windows"], stats["window_sites"]),
              file=sys.stderr, flush=True)
    _save_loo(args, ll, parts, sample_names, pops, IDs, say, "_downsampled" if scored else "")


def _run_fit_windowed(args, ctx, W, IDs, pops, say, summary):
    """--get_reference_af on a file that does not fit (or WGSASSIGN_WINDOW_SITES): fitted window by window in rounds.  With --ne_obs
    (WGSASSIGN_NE_WINDOW_SITES) one pass for the Fisher information follows, over the frequencies just written; with --loo
    (WGSASSIGN_LOO_WINDOW_SITES, or beside --ne_obs) the leave-one-out run, in the same windows."""
    import numpy as np

    from . import emMAF, fisher
    af, iters = emMAF.emMAF_windowed(args.beagle, IDs, args.maf_iter, args.maf_tole, W, out=args.out + ".pop_af.npy", ctx=ctx)
    info, stats = emMAF.emMAF_windowed.info, emMAF.emMAF_windowed.stats
    say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
    summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
    say("Parsing reference population ID file.")
    _say_converged(iters, say)
    print("wgsassign_amd: fitted in %d rounds of %d windows of %d sites" % (stats["rounds"], stats["windows"], stats["window_sites"]),
          file=sys.stderr, flush=True)
    del af
    _save_names(args, pops, say)
    if args.ne_obs:
        say("Estimating Fisher information.")
        A = np.load(args.out + ".pop_af.npy", mmap_mode="r")
        f_obs, ne_obs, ne_obs_mean, ne_ind = fisher.fisher_obs_windowed(args.beagle, A, IDs, W, out=args.out, ctx=ctx)
        del A, f_obs, ne_obs
        stats = fisher.fisher_obs_windowed.stats
        print("wgsassign_amd: Fisher information in %d windows of %d sites" % (stats["windows"], stats["window_sites"]), file=sys.stderr,
              flush=True)
        _save_ne_obs(args, pops, say, ne_obs_mean, lambda: ne_ind)
    if args.loo:
        _loo_windowed(args, ctx, W, IDs, pops, info["sample_names"], iters, say)


def _run_loo_ds_windowed(args, ctx, W, IDs, pops, sample_names, keep_ref, keep_ds, say):
    """--get_reference_af --loo --loo_downsampled_beagle on files that do not fit (or WGSASSIGN_LOO_DS_WINDOW_SITES), after the names
    passes and the two site masks of the resident run: the fit over the kept sites of the reference file in windows, then the
    leave-one-out run in the same windows with the downsampled file's windows scored beside them."""
    from . import emMAF
    say("Parsing reference population ID file.")
    assert (len(sample_names) == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    af, iters = emMAF.emMAF_windowed(args.beagle, IDs, args.maf_iter, args.maf_tole, W, out=args.out + ".pop_af.npy", ctx=ctx, keep=keep_ref)
    _say_converged(iters, say)
    del af
    _save_names(args, pops, say)
    _loo_windowed(args, ctx, W, IDs, pops, sample_names, iters, say, keep_ref, keep_ds)


def _run_z_windowed(args, flavour, ctx, plan, IDs, group_of, say, summary):
    """--get_assignment_z_score or --get_reference_z_score alone (flavour: "assignment" / "reference") on files that do not fit (or
    WGSASSIGN_Z_WINDOW_SITES / WGSASSIGN_ZREF_WINDOW_SITES): passes over the Beagle file and the depth file in site windows; the
    checks, lines and file of the resident run in their order."""
    import numpy as np

    from . import reader_cy, zscore
    W, batch = plan
    assignment = flavour == "assignment"
    index, _, m = reader_cy.ensure_index(args.beagle)
    with reader_cy.BeagleStream(args.beagle, threads=1) as st:
        n = st.n
    assert os.path.isfile(args.pop_af_IDs), "Population ID file does not exist!!"
    if assignment:
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
    if assignment:
        pops = np.loadtxt(args.pop_names, dtype="str")
    assert (n == IDs.shape[0]), "Number of individuals in beagle and reference ID file do not match!"
    if args.allele_count_threshold is not None:
        assert (args.allele_count_threshold >= 0), "Allele count threshold needs to be greater than/equal to 0!"
    thresholds = (args.allele_count_threshold or 0, args.single_read_threshold)
    ind_start, ind_end = zscore.ind_range(n, args.ind_start, args.ind_end)
    lines = []
    windowed = dict(window_sites=W, say=lines.append, counts=majmin is not None, majmin=majmin, batch=batch, ctx=ctx)
    depth_file = args.ind_counts_file or args.ind_ad_file
    if assignment:
        run = zscore.assignment_z_scores_windowed
        z_out = run(args.beagle, depth_file, A, IDs, np.atleast_1d(pops), *thresholds, ind_start, ind_end, **windowed)
    else:
        run = zscore.reference_z_scores_windowed
        z_out = run(args.beagle, depth_file, IDs, group_of, args.maf_iter, args.maf_tole, *thresholds, ind_start, ind_end, **windowed)
    info, stats = run.info, run.stats
    say("Loaded " + str(info["m"]) + " sites and " + str(info["n"]) + " individuals.")
    summary(info["sample_names"], info["m"], [(info["site_names"][:4], info["site_names"][-4:])])
    say("Parsing population ID file.")
    if assignment:
        say("Parsing population allele frequency file.")
    say("Parsing individual allele depths file.")
    for ln in lines:
        say(ln)
    if assignment:
        print("wgsassign_amd: z-scores in %d rounds of 2 passes over %d windows of %d sites (%d bytes downloaded)" %
              (stats["rounds"], stats["windows"], stats["window_sites"], stats["downloaded_bytes"]), file=sys.stderr, flush=True)
    else:
        print("wgsassign_amd: reference z-scores in %d rounds of individuals, %d passes over %d windows of %d sites (%d bytes downloaded)" %
              (stats["rounds"], stats["passes"], stats["windows"], stats["window_sites"], stats["downloaded_bytes"]), file=sys.stderr, flush=True)
    name = ".z_ind.txt" if assignment else ".reference_z_ind.txt"
    np.savetxt(args.out + name, z_out, fmt="%.7f")
    say("Saved " + str(ind_end - ind_start) + " individual z-scores as " + str(args.out) + name + " (text)")


def _run(args, comm):
    """The hot-path options on device-resident data.  Under torchrun (one process per GPU) the SNPs are
    sharded over the ranks: every rank parses and holds only its contiguous SNP range; the EM convergence sums,
    the serial-chain carry and the n x K log-likelihood sums cross ranks through one sum
    all-reduce (RCCL); rank 0 writes the reference's output files.  On one rank, options that a windowed route covers
    (ROUTES) run in site windows when their files do not fit the device or their variable asks for it."""
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
        _run_score_windowed(args, ctx, W, say, summary)
        comm.barrier()
        return
    for ask in (_fit_window_sites, _loo_window_sites, _ne_window_sites):     # (each asked only when those before it said None)
        W = ask(args, comm, ctx)
        if W is not None:
            _run_fit_windowed(args, ctx, W, IDs, pops, say, summary)
            comm.barrier()
            return
    for flavour, ask in (("assignment", _z_window_sites), ("reference", _zref_window_sites)):
        plan = ask(args, comm, ctx)
        if plan is not None:
            _run_z_windowed(args, flavour, ctx, plan, IDs, group_of, say, summary)
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
            del names_ref, names_ds, kept_ref       # (the names of both files still live on the host)
            _run_loo_ds_windowed(args, ctx, W_ds, IDs, pops, sample_names, keep_ref, keep_ds, say)
            comm.barrier()
            return
        try:
            beagle, _, site_names, m = reader_cy.stream_to_device(args.beagle, group_of, n_groups, ctx=ctx, rank=comm.rank,
                                                                  world=comm.world, keep=keep_ref, comm=comm)
            scored, _, _, _ = reader_cy.stream_to_device(args.loo_downsampled_beagle, group_of, n_groups, ctx=ctx,
                                                         rank=comm.rank, world=comm.world, keep=keep_ds, comm=comm)
        except RuntimeError as e:
            _raise_hinted(e, args, comm.world)
    else:
        try:
            beagle, sample_names, site_names, m = reader_cy.stream_to_device(
                args.beagle, group_of, n_groups, ctx=ctx, rank=comm.rank, world=comm.world, comm=comm, names="ends")
        except RuntimeError as e:
            _raise_hinted(e, args, comm.world)
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
        _save_names(args, pops, say, root)
        if args.ne_obs:                      # per-SNP quantities shard trivially; rank 0 assembles and writes
            say("Estimating Fisher information.")
            f_loc, ne_loc = fisher.fisher_obs(None, af, IDs, args.threads, beagle=beagle)
            f_obs, ne_obs = comm.gather_rows(f_loc), comm.gather_rows(ne_loc)
            # np.mean's running float32 total is handed from SNP shard to SNP shard (fisher.fisher_obs_ind)
            _save_ne_obs(args, pops, say, np.mean(ne_obs, axis=0) if root else None,
                         lambda: fisher.fisher_obs_ind(None, af, IDs, args.threads, beagle=beagle, comm=comm, m_total=m),
                         per_locus=(f_obs, ne_obs), root=root)

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
                _save_loo(args, ll, parts, sample_names, pops, IDs, say, "_downsampled" if scored is not None else "")

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
