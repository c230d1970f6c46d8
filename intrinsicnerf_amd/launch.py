"""Run the reference's OWN entry scripts on the MI355X render path, without editing a line of them:

    python -m intrinsicnerf_amd.launch  <IntrinsicNeRF>/object_level/run_nerf.py  --config configs/chair.txt [...]
    python -m intrinsicnerf_amd.launch  <IntrinsicNeRF>/train_SSR_main.py  --config_file SSR/configs/SSR_room0_config.yaml [...]

The reference is pure Python: the "operator interface" of its render path is a handful of module-level functions and three
trainer methods.  The launcher loads the script as a module (everything above its
``if __name__ == '__main__':`` block), rebinds exactly those names to this package's mirrors - in the namespaces the
reference's own code looks them up in - and then executes the script's own main block (seeds, default tensor type,
``train()``) as if it had been started with ``python``.  What INTEGRATION.md section A describes as two edits, done at run time.

  object_level/run_nerf.py    (run_nerf.py:32-139, 359-528; run_nerf_helpers.py:195-445)
      run_network, batchify_rays, render, render_rays, raw2outputs, NeRF, get_embedder, Embedder, sample_pdf, get_rays,
      get_rays_np, ndc_rays  [+ render_path, to8b with --inerf-render-path]
      ``create_nerf`` stays the reference's: its ``network_query_fn`` lambda is recognised structurally
      (object_level._as_network_query) once ``run_network`` in the script's namespace is this package's.
  train_SSR_main.py           (SSR/training/trainer.py:693-846; SSR/models/*.py; SSR/training/cluster.py:73-98)
      SSRTrainer.render_rays / volumetric_rendering / create_ssr <- ssr.SSRRenderMixin's; run_network, raw2outputs,
      sample_pdf, create_rays, Semantic_NeRF, get_embedder in every SSR module that holds them; the two cluster lookups.

``--inerf-cluster-fit`` (opt-in) also moves the mean-shift fit of the albedo clusters onto the GPU: the reference's
``Cluster.update_center`` / ``Cluster_Manager.update_center`` become ``cluster.fit_cluster`` / ``cluster.update_center``
(csrc/cluster_fit.hip), and with ``--inerf-render-path`` the mirrors' ``render_path`` builds the package's
``Cluster_Manager``.

``--inerf-cluster-refresh`` (opt-in; takes effect only together with ``--inerf-render-path``, and implies ``--inerf-cluster-fit``)
keeps the whole cluster-refresh pass of ``render_path(update_cluster=True)`` on the device (``refresh.ClusterRefresh``,
csrc/refresh.hip): the mirrors' ``render_path`` gets ``refresh=`` (object level) and ``SSRTrainer.cluster_refresh`` (SSR), each
a ``ClusterRefresh`` - every second albedo pixel goes into the fit's sample table as its frame is rendered, the fit reads the table
where it is, and ``c###.png`` / ``edit###.png`` come back as 8-bit images.  Same files, same returned manager.

``--inerf-losses`` (opt-in) moves the intrinsic loss terms onto the GPU kernels of csrc/losses.hip: ``compute_intrinsic_loss``
becomes ``losses.compute_intrinsic_loss`` where the trainers look it up - ``run_nerf.py``'s own namespace
(``from run_nerf_helpers import *``, called at run_nerf.py:977,1007) and ``SSR.training.trainer`` (imported by name at
trainer.py:15, called at :924,937).  Six scalars in the reference's order through one autograd node; the trainers' weighted
sums and ``loss.backward()`` stay their own lines.

``--inerf-adam`` (opt-in) replaces the optimizer the trainers build - ``torch.optim.Adam`` at run_nerf.py:304 and trainer.py:842 -
by ``optim.Adam`` (csrc/adam.hip: one launch of the library per step) over the same parameter groups, with the same
``lr / betas / eps`` and whatever state a checkpoint loaded into it: ``create_nerf`` in ``run_nerf.py``'s namespace is wrapped
(it returns the optimizer as its fifth value, run_nerf.py:356, after run_nerf.py:325 loaded the checkpoint) and so is
``SSRTrainer.create_ssr`` (it assigns ``self.optimizer``, trainer.py:848).  Nothing in ``torch.optim`` is patched; the
trainers' ``optimizer.zero_grad()``, ``optimizer.step()``, learning-rate decay and ``optimizer.state_dict()`` stay their lines.

``--inerf-batches`` (opt-in) assembles the SSR training batch in one launch of csrc/batch.hip: ``SSRTrainer.sample_data``
(trainer.py:627-691) becomes ``ssr.SSRRenderMixin.sample_data`` - the draws stay the reference's own ``sampling_index``
(rays.py:153-172), so a seeded run selects the reference's pixels; every gather is the one launch.  The object-level batch code
is inline in ``train()`` (run_nerf.py:886-938) and cannot be rebound from outside: for ``run_nerf.py`` the flag only says so, once;
INTEGRATION.md has its three-line replacement by ``batches.ObjectBatcher.next(i)``.

``--inerf-draws`` (opt-in) draws the training step's random tensors - the stratified jitter, the density noise of both passes and
the inverse-CDF variates - inside the kernels (csrc/draws.h, ``draws.DrawState``) instead of with ``torch.rand`` / ``torch.randn``:
``create_nerf`` in ``run_nerf.py``'s namespace is wrapped so that ``render_kwargs_train["draws"]`` holds a ``DrawState``, and
``SSRTrainer.draws`` yields one per trainer.  Both are created on first use with ``seed = torch.initial_seed()``, i.e. after the script's
own seeding.  The draws are this package's counter-based ones, not torch's streams: a seeded run is reproducible, and its renders do
not depend on ``chunk``.  Without the flag nothing of this is bound.

``--inerf-eval`` (opt-in) rebinds the reference's two metric functions - ``calculate_segmentation_metrics`` and
``calculate_depth_metrics`` - to ``evaluation``'s (csrc/eval.hip: one accumulate launch, finished on the host in float64) in both
``SSR.training.trainer`` (which holds them by value, trainer.py:15) and ``SSR.training.training_utils``.  That alone lets the
reference's validation step run on a current numpy: its own function uses ``np.float``, which numpy 1.24 removed.  Wiring an
``evaluation.FrameEvaluator`` into the unedited trainer is out of scope - which ray set pairs with which targets is the trainer's
knowledge (INTEGRATION.md has the four lines).  ``run_nerf.py`` has no metric functions: the flag only says so, once.

``--inerf-frame-products`` (opt-in; takes effect only together with ``--inerf-render-path``) makes every 8- and 16-bit image of the
mirrors' ``render_path`` on the device (``frames.FrameProducts``, csrc/frame_vis.hip): the mirrors get ``products=`` (object level)
and ``SSRTrainer.frame_products`` (SSR).  The SSR trainer's ``vis_deps`` / ``vis_entropys`` and its ``vis_depth_*`` / ``vis_entropy_*``
files then need no imgviz at run time.

``--inerf-frame-png`` (opt-in; implies ``--inerf-frame-products``) also encodes those images to PNG files on the device
(``frames.FrameProducts(encode=True)``, csrc/png.hip): ``render_path(savedir=...)`` then writes the bytes it is handed - the same file
names, the same pixels, other file bytes than the host encoder's.

``--inerf-movies`` (opt-in) binds the name ``imageio`` in the reference's modules that call ``imageio.mimwrite`` (run_nerf.py:822,
:1051-1052; trainer.py:1088-1093, :1169-1174; the two dataset modules) to a small proxy: ``mimwrite(path, frames, fps=, quality=)``
writes a Motion-JPEG AVI file on the device (``frames.write_movie``, csrc/jpeg.hip) under the path with its extension replaced by
``.avi`` and says so once; imageio's ``quality`` 0 .. 10 becomes the JPEG quality ``50 + 5 * quality`` (8 -> 90, 10 -> 100; None -> 75,
imageio's default 5).  Every other attribute forwards to the real imageio when there is one; on a host without it the proxy also
stands in for the module, so that the scripts' ``import imageio`` succeeds.

``prepare(script)`` does everything but run the main block and returns the module (used by the tests).
"""
import ast
import importlib
import os
import sys
import types

OBJECT_SYMBOLS = ("run_network", "batchify_rays", "render", "render_rays", "raw2outputs", "NeRF", "get_embedder", "Embedder",
                  "sample_pdf", "get_rays", "get_rays_np", "ndc_rays")
OBJECT_OPTIONAL = ("render_path", "to8b")
SSR_METHODS = ("render_rays", "volumetric_rendering", "create_ssr")
SSR_SYMBOLS = ("run_network", "raw2outputs", "sample_pdf", "create_rays", "Semantic_NeRF", "get_embedder", "Embedder")
SSR_MODULES = ("SSR.training.trainer", "SSR.models.model_utils", "SSR.models.rays", "SSR.models.semantic_nerf")


def _split_main(source, filename):
    """(code of everything but the ``if __name__ == '__main__':`` blocks, code of their bodies) of a script."""
    tree = ast.parse(source, filename)
    body, main = [], []
    for node in tree.body:
        is_main = (isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.left, ast.Name)
                   and node.test.left.id == "__name__" and len(node.test.comparators) == 1
                   and isinstance(node.test.comparators[0], ast.Constant) and node.test.comparators[0].value == "__main__")
        (main if is_main else body).append(node)
    main_body = [stmt for node in main for stmt in node.body]
    mk = lambda nodes: compile(ast.fix_missing_locations(ast.Module(body=nodes, type_ignores=[])), filename, "exec")
    return mk(body), mk(main_body)


def _kind(script):
    name = os.path.basename(script)
    if name == "run_nerf.py":
        return "object"
    if name == "train_SSR_main.py":
        return "ssr"
    raise SystemExit(f"intrinsicnerf_amd.launch: {name}: expected the reference's object_level/run_nerf.py or train_SSR_main.py")


def rebind_cluster_fit(module_name):
    """The GPU mean-shift fit onto the reference's ``Cluster`` / ``Cluster_Manager`` of ``module_name`` (if imported):
    returns {qualified class name: [methods bound]}."""
    from . import cluster as inerf_cluster
    mod = sys.modules.get(module_name)
    bound = {}
    if mod is None:
        return bound
    if hasattr(mod, "Cluster"):
        mod.Cluster.update_center = inerf_cluster.fit_cluster
        bound[module_name + ".Cluster"] = ["update_center"]
    if hasattr(mod, "Cluster_Manager"):
        mod.Cluster_Manager.update_center = inerf_cluster.update_center
        bound[module_name + ".Cluster_Manager"] = ["update_center"]
    return bound


LOSS_SYMBOL = "compute_intrinsic_loss"


def _with_inerf_adam_nerf(create_nerf):
    """``create_nerf`` whose fifth return value (run_nerf.py:356) is ``optim.Adam`` in place of the torch.optim.Adam it built."""
    import functools

    @functools.wraps(create_nerf)
    def create_nerf_inerf_adam(*args, **kwargs):
        from . import optim
        out = list(create_nerf(*args, **kwargs))
        out[4] = optim.from_torch(out[4])
        return tuple(out)
    return create_nerf_inerf_adam


def _with_inerf_adam_ssr(create_ssr):
    """``create_ssr`` that leaves ``optim.Adam`` in ``self.optimizer`` (trainer.py:848)."""
    import functools

    @functools.wraps(create_ssr)
    def create_ssr_inerf_adam(self, *args, **kwargs):
        from . import optim
        out = create_ssr(self, *args, **kwargs)
        self.optimizer = optim.from_torch(self.optimizer)
        return out
    return create_ssr_inerf_adam


def _with_inerf_draws_nerf(create_nerf):
    """``create_nerf`` whose ``render_kwargs_train`` (first return value, run_nerf.py:356) carries ``draws``: a DrawState seeded with
    ``torch.initial_seed()`` on the device of the networks' parameters."""
    import functools

    @functools.wraps(create_nerf)
    def create_nerf_inerf_draws(*args, **kwargs):
        import torch
        from . import draws
        out = list(create_nerf(*args, **kwargs))
        params = list(out[0]["network_fn"].parameters())
        out[0]["draws"] = draws.DrawState(torch.initial_seed(), params[0].device)
        return tuple(out)
    return create_nerf_inerf_draws


class _TrainerDraws:
    """``SSRTrainer.draws``: one DrawState per trainer, created when the render path first asks for it (the networks exist then and
    the script has seeded torch), seed = ``torch.initial_seed()``."""

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        import torch
        from . import draws
        state = draws.DrawState(torch.initial_seed(), next(obj.ssr_net_coarse.parameters()).device)
        obj.__dict__["draws"] = state                  # (a non-data descriptor: the instance attribute wins from now on)
        return state


def rebind_object_level(namespace, with_render_path=False, cluster_fit=False, losses=False, adam=False, draws=False, cluster_refresh=False,
                        frame_products=False, frame_png=False):
    """The object-level mirrors into ``namespace`` (a module's ``__dict__``): returns the names it bound."""
    from . import object_level
    cluster_fit = cluster_fit or (cluster_refresh and with_render_path)          # the refresh pass fits on the GPU
    frame_products = frame_products or frame_png       # the files are encoded from the products' planes
    names = OBJECT_SYMBOLS + (OBJECT_OPTIONAL if with_render_path else ()) + ((LOSS_SYMBOL,) if losses else ())
    for name in names:
        namespace[name] = getattr(object_level, name)
    if adam:
        namespace["create_nerf"] = _with_inerf_adam_nerf(namespace["create_nerf"])
        names = names + ("create_nerf",)
    if draws:
        namespace["create_nerf"] = _with_inerf_draws_nerf(namespace["create_nerf"])
        if "create_nerf" not in names:
            names = names + ("create_nerf",)
    if cluster_fit:
        rebind_cluster_fit("cluster")                  # run_nerf.py:24 `from cluster import Cluster, Cluster_Manager`
    if with_render_path and "Cluster_Manager" in namespace:
        # run_nerf.py:818,1071 call render_path(update_cluster=True): the reference's own class (run_nerf.py:24, :218) is
        # handed to the mirror as its factory - the package's GPU-fitted one under --inerf-cluster-fit
        import functools
        from . import cluster as inerf_cluster
        factory = inerf_cluster.Cluster_Manager if cluster_fit else namespace["Cluster_Manager"]
        extra = {}
        if cluster_refresh:
            from . import refresh
            extra["refresh"] = refresh.ClusterRefresh(manager_factory=factory)
        if frame_products:
            from . import frames
            extra["products"] = frames.FrameProducts(encode=frame_png)
        namespace["render_path"] = functools.partial(object_level.render_path, cluster_manager_factory=factory, **extra)
    elif with_render_path and frame_products:
        import functools
        from . import frames
        namespace["render_path"] = functools.partial(object_level.render_path, products=frames.FrameProducts(encode=frame_png))
    return names


MOVIE_MODULES = ("run_nerf", "SSR.training.trainer", "SSR.datasets.replica.replica_datasets", "SSR.datasets.scannet.scannet_datasets")


def movie_quality(quality):
    """imageio's ``quality`` (0 .. 10, None: its default 5) as a JPEG quality: 50 + 5 * quality, so 8 -> 90 and 10 -> 100."""
    q = 5.0 if quality is None else float(quality)
    if not 0 <= q <= 10:
        raise ValueError(f"quality = {quality}: imageio takes 0 .. 10")
    return int(round(50 + 5 * q))


class _MovieProxy:
    """Stands where a reference module holds ``imageio``: ``mimwrite`` / ``mimsave`` write Motion-JPEG AVI files on the device,
    everything else is the real module's (AttributeError when there is none)."""

    def __init__(self, real):
        self.__dict__["_real"], self.__dict__["_told"] = real, False

    def mimwrite(self, path, frames_, fps=30, quality=None, **ignored):
        from . import frames
        target = os.path.splitext(os.fspath(path))[0] + ".avi"
        if not self._told:
            print(f"intrinsicnerf_amd.launch: --inerf-movies writes Motion-JPEG AVI files on the device: {path} becomes {target}",
                  file=sys.stderr)
            self.__dict__["_told"] = True
        return frames.write_movie(target, frames_, fps=fps, quality=movie_quality(quality))

    mimsave = mimwrite

    def __getattr__(self, name):
        if self._real is None:
            raise AttributeError(f"imageio is not installed: the --inerf-movies proxy has mimwrite alone, not {name!r}")
        return getattr(self._real, name)


def movie_proxy(real="import"):
    """The proxy around ``real`` (default: imageio if it can be imported, else nothing)."""
    if isinstance(real, str):
        try:
            real = importlib.import_module("imageio")
        except ImportError:
            real = None
        if isinstance(real, _MovieProxy):
            return real
    return _MovieProxy(real)


def install_movie_stand_in():
    """On a host without imageio the proxy is also the module ``imageio``, so that the scripts' imports succeed."""
    try:
        importlib.import_module("imageio")
    except ImportError:
        sys.modules["imageio"] = movie_proxy(None)


def rebind_movies(extra_modules=()):
    """``imageio`` -> the proxy in every loaded module of MOVIE_MODULES (and ``extra_modules``) that holds it: [module names]."""
    proxy, bound = movie_proxy(), []
    for mod in [sys.modules.get(n) for n in MOVIE_MODULES] + list(extra_modules):
        if mod is not None and hasattr(mod, "imageio") and mod.__name__ not in bound:
            mod.imageio = proxy
            bound.append(mod.__name__)
    return bound


EVAL_SYMBOLS = ("calculate_segmentation_metrics", "calculate_depth_metrics")
EVAL_MODULES = ("SSR.training.trainer", "SSR.training.training_utils")


def rebind_eval():
    """The two metric functions onto the (already imported) reference modules that hold them: {module name: [names bound]}."""
    from . import evaluation
    bound = {}
    for mod_name in EVAL_MODULES:
        mod = sys.modules.get(mod_name)
        if mod is None:
            continue
        for name in EVAL_SYMBOLS:
            setattr(mod, name, getattr(evaluation, name))
        bound[mod_name] = list(EVAL_SYMBOLS)
    return bound


def rebind_ssr(with_render_path=False, cluster_fit=False, losses=False, adam=False, batches=False, draws=False, cluster_refresh=False, evaluate=False,
               frame_products=False, frame_png=False):
    """The SSR mirrors into the (already imported) reference modules; returns {module name: [names bound]}."""
    from . import cluster as inerf_cluster, ssr
    cluster_fit = cluster_fit or (cluster_refresh and with_render_path)          # the refresh pass fits on the GPU
    bound = {}
    trainer = sys.modules["SSR.training.trainer"]
    methods = SSR_METHODS + (("render_path",) if with_render_path else ())
    for name in methods:
        setattr(trainer.SSRTrainer, name, getattr(ssr.SSRRenderMixin, name))
    for extra in ("return_raw", "check_numerics", "draws"):          # what the mixin's methods read besides the trainer's attributes
        setattr(trainer.SSRTrainer, extra, getattr(ssr.SSRRenderMixin, extra))
    if with_render_path and hasattr(trainer, "Cluster_Manager"):
        # trainer.py:1065 renders with update_cluster = not self.no_cluster: the fitting is the reference's class (trainer.py:16, :1416-1418)
        factory = inerf_cluster.Cluster_Manager if cluster_fit else trainer.Cluster_Manager
        trainer.SSRTrainer.cluster_manager_factory = staticmethod(factory)
        if cluster_refresh:                            # read by the mirror's render_path (ssr.SSRRenderMixin.cluster_refresh is None)
            from . import refresh
            trainer.SSRTrainer.cluster_refresh = refresh.ClusterRefresh(manager_factory=factory)
    bound["SSR.training.trainer.SSRTrainer"] = list(methods)
    if with_render_path and (frame_products or frame_png):      # read by the mirror's render_path (ssr.SSRRenderMixin.frame_products is None)
        from . import frames
        trainer.SSRTrainer.frame_products = frames.FrameProducts(encode=frame_png)
        bound["SSR.training.trainer.SSRTrainer"].append("frame_products")
    for mod_name in SSR_MODULES:
        mod = sys.modules.get(mod_name)
        if mod is None:
            continue
        here = [n for n in SSR_SYMBOLS if hasattr(mod, n)]
        for n in here:
            setattr(mod, n, getattr(ssr, n))
        bound[mod_name] = here
    cl = sys.modules.get("SSR.training.cluster")
    if cl is not None and hasattr(cl, "Cluster_Manager"):               # cluster.py:73-98: one HIP launch for all classes
        cl.Cluster_Manager.dest_color = inerf_cluster.dest_color
        cl.Cluster_Manager.dest_class = inerf_cluster.dest_class
        bound["SSR.training.cluster.Cluster_Manager"] = ["dest_color", "dest_class"]
    if cluster_fit:
        for name, methods in rebind_cluster_fit("SSR.training.cluster").items():
            bound.setdefault(name, []).extend(methods)
    if losses:                                         # trainer.py:15 holds the function by value; step() looks it up in its module
        setattr(trainer, LOSS_SYMBOL, getattr(ssr, LOSS_SYMBOL))
        bound.setdefault("SSR.training.trainer", []).append(LOSS_SYMBOL)
    if adam:                                           # (create_ssr is the mixin's by now: the wrapper goes around that one)
        trainer.SSRTrainer.create_ssr = _with_inerf_adam_ssr(trainer.SSRTrainer.create_ssr)
    if batches:                                        # trainer.py:627-691; its draws stay SSR.models.rays.sampling_index
        trainer.SSRTrainer.sample_data = ssr.SSRRenderMixin.sample_data
        bound["SSR.training.trainer.SSRTrainer"].append("sample_data")
    if draws:                                          # (without the flag SSRTrainer.draws is the mixin's default, None)
        trainer.SSRTrainer.draws = _TrainerDraws()
        bound["SSR.training.trainer.SSRTrainer"].append("draws")
    if evaluate:                                       # trainer.py:15 imported training_utils and holds both functions by value
        for mod_name, names in rebind_eval().items():
            bound.setdefault(mod_name, []).extend(names)
    return bound


_told_object_batches = False


def _object_batches_notice():
    """Said once: run_nerf.py builds its batch inline in train() (run_nerf.py:886-938); nothing there can be rebound."""
    global _told_object_batches
    if not _told_object_batches:
        print("intrinsicnerf_amd.launch: --inerf-batches has no effect on run_nerf.py: its batch code is inline in train() "
              "(run_nerf.py:886-938).  Replace those lines by batches.ObjectBatcher.next(i) (INTEGRATION.md).", file=sys.stderr)
        _told_object_batches = True


_told_object_eval = False


def _object_eval_notice():
    """Said once: run_nerf.py computes no validation metrics beyond its inline PSNR; there is nothing to rebind."""
    global _told_object_eval
    if not _told_object_eval:
        print("intrinsicnerf_amd.launch: --inerf-eval has no effect on run_nerf.py: it has no metric functions "
              "(calculate_segmentation_metrics / calculate_depth_metrics belong to train_SSR_main.py).  evaluation.image_mse_psnr "
              "serves a loop of your own (INTEGRATION.md).", file=sys.stderr)
        _told_object_eval = True


def prepare(script, with_render_path=False, cluster_fit=False, losses=False, adam=False, batches=False, draws=False, cluster_refresh=False,
            evaluate=False, frame_products=False, frame_png=False, movies=False):
    """Load the reference script as a module (without its main block), rebind the render path, return (module, main code)."""
    if movies:
        install_movie_stand_in()
    script = os.path.abspath(script)
    kind = _kind(script)
    root = os.path.dirname(script)
    if root not in sys.path:
        sys.path.insert(0, root)                       # what `python script.py` does: the script's directory leads sys.path
    with open(script, "r") as fh:
        body, main = _split_main(fh.read(), script)
    mod = types.ModuleType("run_nerf" if kind == "object" else "train_SSR_main")
    mod.__file__ = script
    sys.modules[mod.__name__] = mod
    exec(body, mod.__dict__)
    products = dict(frame_products=True) if frame_products or frame_png else {}      # (only when given, as `evaluate` below)
    if frame_png:
        products["frame_png"] = True
    if kind == "object":
        mod.__dict__["__inerf_bound__"] = rebind_object_level(mod.__dict__, with_render_path, cluster_fit, losses, adam, draws, cluster_refresh,
                                                              **products)
        if batches:
            _object_batches_notice()
        if evaluate:
            _object_eval_notice()
    else:
        importlib.import_module("SSR.training.trainer")
        extra = dict(evaluate=True) if evaluate else {}           # (only when given: a stand-in rebind_ssr of the older signature keeps working)
        extra.update(products)
        mod.__dict__["__inerf_bound__"] = rebind_ssr(with_render_path, cluster_fit, losses, adam, batches, draws, cluster_refresh, **extra)
    if movies:
        mod.__dict__["__inerf_movies__"] = rebind_movies([mod])
    return mod, main


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    with_render_path = "--inerf-render-path" in argv
    if with_render_path:
        argv.remove("--inerf-render-path")
    cluster_fit = "--inerf-cluster-fit" in argv
    if cluster_fit:
        argv.remove("--inerf-cluster-fit")
    cluster_refresh = "--inerf-cluster-refresh" in argv
    if cluster_refresh:
        argv.remove("--inerf-cluster-refresh")
    losses = "--inerf-losses" in argv
    if losses:
        argv.remove("--inerf-losses")
    adam = "--inerf-adam" in argv
    if adam:
        argv.remove("--inerf-adam")
    batches = "--inerf-batches" in argv
    if batches:
        argv.remove("--inerf-batches")
    draws = "--inerf-draws" in argv
    if draws:
        argv.remove("--inerf-draws")
    evaluate = "--inerf-eval" in argv
    if evaluate:
        argv.remove("--inerf-eval")
    frame_products = "--inerf-frame-products" in argv
    if frame_products:
        argv.remove("--inerf-frame-products")
    frame_png = "--inerf-frame-png" in argv
    if frame_png:
        argv.remove("--inerf-frame-png")
        frame_products = True                          # the files are encoded from the products' planes
    movies = "--inerf-movies" in argv
    if movies:
        argv.remove("--inerf-movies")
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    script = argv[0]
    from . import _capi
    _capi.lib()                                        # fail now, and loudly, if the HIP library is missing
    # (positional as before for the first two; the loss flag only when given, so a two-flag `prepare` stand-in keeps working)
    extra = dict(adam=True) if adam else {}            # (by keyword and only when given, for the same reason)
    if batches:
        extra["batches"] = True
    if draws:
        extra["draws"] = True
    if cluster_refresh:
        extra["cluster_refresh"] = True
    if evaluate:
        extra["evaluate"] = True
    if frame_products:
        extra["frame_products"] = True
    if frame_png:
        extra["frame_png"] = True
    if movies:
        extra["movies"] = True
    if extra:
        mod, main_code = prepare(script, with_render_path, cluster_fit, losses, **extra)
    else:
        mod, main_code = prepare(script, with_render_path, cluster_fit, losses) if losses else prepare(script, with_render_path, cluster_fit)
    sys.argv = [script] + argv[1:]                     # the script's own argument parser sees its own command line
    mod.__dict__["__name__"] = "__main__"
    exec(main_code, mod.__dict__)
    return 0


if __name__ == "__main__":
    sys.exit(main())
