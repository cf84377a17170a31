"""Executors with the reference's interface (network/executors.py:26-268): `train(batch, calc_loss)`,
`test(batch, eval_pred)`, `calc_loss`, `eval`, `save`.  The class for a model is found by name:
network.models.X <-> network.executors.X (train.py of the reference, line 242)."""
import numpy as np
import torch

from .. import augment, chamfer, components, evaluate, mesh, parallel, refine as RF, render, resize, s2loss, simplify, utils
from . import losses as L


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def chamfer_distance(x, y):
    """Symmetric mean squared nearest-neighbour distance between point sets [B,N,3], [B,M,3]
    (what pytorch3d.loss.chamfer_distance returns with default arguments)."""
    d = torch.cdist(x, y) ** 2
    return d.min(2)[0].mean(1).mean() + d.min(1)[0].mean(1).mean(), None


class _TrainImages:
    """The 'rgb_image' of a training batch on the device.  A uint8 [B,H,W,3] batch (--augment hip: the datasets hand out
    the files' pixels) is flipped, jittered and converted there in one launch (augment.apply), with parameters drawn per
    batch from a generator seeded once per process (per rank); a float batch is copied as it is.  A resize.RaggedImages
    (images of different sizes, from Datasets.collate) is also resized there to img_res x img_res (resize.apply), behind the
    flip and the jitter of the same draws."""

    def __init__(self, config):
        self.flip = bool(getattr(config, "random_h_flip", False))
        self.jitter = bool(getattr(config, "color_jitter", False))
        self.img_res = int(getattr(config, "img_res", 224))
        self.generator = torch.Generator().manual_seed(333 + parallel.world_info()[0])

    def __call__(self, img, dev):
        if isinstance(img, resize.RaggedImages):
            params = augment.draw_params(len(img), self.flip, self.jitter, self.generator)
            return resize.apply(img.to(dev), self.img_res, self.img_res, params)
        if img.dtype != torch.uint8:
            return img.to(dev)
        return augment.apply(img.to(dev), augment.draw_params(img.shape[0], self.flip, self.jitter, self.generator))


# --render_pred -> (the model's own view, the three canonical views)
RENDER_VIEWS = {"none": (False, False), "view": (True, False), "canonical": (False, True), "both": (True, True)}
VIEW_ALPHA = 0.65            # the mesh's opacity over the input image in the "view" picture


class CoarseNet:
    def __init__(self, config, model):
        self.train_images = _TrainImages(config)
        self.loss_fn = chamfer_distance
        self.use_cuda = config.cuda
        self.model = model
        self.coarse_points = config.coarse_point_density

    def calc_loss(self, pred, gt):
        # on the GPU the HIP loss (include/list_loss.h: no B x N x M matrix, a deterministic backward); CPU tensors
        # keep the torch path
        loss_fn = chamfer.chamfer_distance if pred.is_cuda else self.loss_fn
        return loss_fn(pred, gt)[0] * 1000

    def _device(self):
        return next(self.model.parameters()).device

    def train(self, batch, calc_loss=True):
        img, gt = self.train_images(batch["rgb_image"], self._device()), batch["pc"].to(self._device())
        pred = self.model(img)
        return pred, {"chamfer_loss": self.calc_loss(pred, gt) if calc_loss else []}

    def test(self, batch, eval_pred=False):
        img, gt = (batch["rgb_image"], batch["pc"]) if isinstance(batch, dict) else batch       # Pix3D hands out a dict
        if gt.dim() == 2:
            gt = gt.unsqueeze(0)
        pred = self.model(img.to(self._device())).detach().cpu()
        return pred, (self.eval(pred, gt) if eval_pred else {})

    def eval(self, pred, gt):
        if pred.shape[0] > 1:
            print("Evaluation of multiple predictions (batch_size > 1) is not allowed.")
            return {}
        return {"chamfer_l2": float(chamfer_distance(pred, gt)[0])}

    def save(self, batch, pred, fname):
        if pred.shape[0] == 1:
            utils.write_obj(fname + "_pred.obj", pred.squeeze(0).numpy(), [])


class LIST:
    def __init__(self, config, model):
        print(self.__class__.__name__, "executor")
        self.model = model
        self.use_cuda = config.cuda
        self.device = getattr(config, "device", None)
        self.test_pointnum = config.test_pointnum
        self.sdf_scale = config.sdf_scale
        self.max_dist = config.sdf_max_dist
        self.query_res = getattr(config, "mcube_znum", None) or config.vox_res
        self.bb_min, self.bb_max, self.vox_res = config.bb_min, config.bb_max, config.vox_res
        self.loss_sdf = L.SDFLoss(self.sdf_scale)
        self.train_images = _TrainImages(config)
        self.stage2_loss = getattr(config, "stage2_loss", "torch")
        if self.stage2_loss not in ("torch", "hip"):
            raise ValueError(f"stage2_loss must be 'torch' or 'hip' (got {self.stage2_loss!r})")
        # coarse-to-fine grid for test(): --refine_stride 0 is the dense grid
        self.refine_stride = getattr(config, "refine_stride", 0) or None
        self.refine_band = getattr(config, "refine_band", None)
        self.last_grid_stats = None
        # --mesh_components K / --mesh_min_faces N: filter the predicted mesh's components; 0 / 0 filters nothing
        self.mesh_components = int(getattr(config, "mesh_components", 0) or 0)
        self.mesh_min_faces = int(getattr(config, "mesh_min_faces", 0) or 0)
        if self.mesh_components < 0 or self.mesh_min_faces < 0:
            raise ValueError(f"mesh_components and mesh_min_faces must be >= 0 (got {self.mesh_components}, "
                             f"{self.mesh_min_faces})")
        self.last_components = None
        # --mesh_simplify C: vertex clustering of the (filtered) predicted mesh on a C^3 grid over the box; 0 is off
        self.mesh_simplify = int(getattr(config, "mesh_simplify", 0) or 0)
        if self.mesh_simplify:
            simplify.check_cells(self.mesh_simplify)
        self.last_simplify = None
        # --render_pred: pictures of the predicted mesh (render.py); 'none' renders nothing
        self.render_pred = getattr(config, "render_pred", "none") or "none"
        if self.render_pred not in RENDER_VIEWS:
            raise ValueError(f"render_pred must be one of {sorted(RENDER_VIEWS)} (got {self.render_pred!r})")
        self.render_size = int(getattr(config, "render_size", 0) or 0) or int(getattr(config, "img_res", 224))
        self.last_transmat = None                   # the camera predict_grid used ([B,4,3]): given, or predicted

    def _device(self):
        return self.device or next(self.model.parameters()).device

    def create_grid(self):
        return utils.create_grid_points_from_bounds(self.bb_min, self.bb_max, self.vox_res)

    def calc_loss(self, pred, gt):
        occ, sdf_pred = pred
        occ_gt, sdf_gt = gt
        w = 0.9                                     # weighted BCE on the occupancy head (executors.py:138-141)
        if self.stage2_loss == "hip" and occ.is_cuda:
            # the local terms in HIP (include/list_s2loss.h): one pass over the volume forward, one backward
            loss = s2loss.stage2_loss(occ, occ_gt, sdf_pred, sdf_gt, self.sdf_scale, w)
            occ_loss = loss["occ_loss"]
        else:
            if not occ_gt.is_floating_point():      # --occ_dtype uint8 (or a bool volume): the same 0 / 1 in occ's dtype
                occ_gt = occ_gt.to(occ.dtype)
            occ_loss = 1000 * (-w * torch.mean(occ_gt * torch.log(occ + 1e-8))
                               - (1 - w) * torch.mean((1 - occ_gt) * torch.log(1 - occ + 1e-8)))
            loss = {"occ_loss": occ_loss}
            loss.update(self.loss_sdf(sdf_pred, sdf_gt))
        rank, world = parallel.world_info()
        if world > 1:
            # One process per GPU holds B_local images.  The reference evaluates SDFLoss over the whole batch
            # (network/losses.py:21-22, nn.DataParallel gathers the outputs): ONE all-gather of the fp32 SDF shards
            # (and of their targets) gives every rank that value; gradients keep flowing through the local term,
            # whose DDP average over the ranks IS the full-batch gradient (equal shards).
            full = self.loss_sdf(parallel.gather_sdf_shards(sdf_pred.detach()),
                                 parallel.gather_sdf_shards(sdf_gt.detach()))
            for k in full:
                loss[k] = parallel.full_batch_value(loss[k], full[k])
            loss["occ_loss"] = parallel.full_batch_value(occ_loss, parallel.all_reduce_mean(occ_loss))
        return loss

    def train(self, batch, calc_loss=True):
        dev = self._device()
        img, points = self.train_images(batch["rgb_image"], dev), batch["points"].to(dev)
        sdf_gt, occ_gt = batch["values"].to(dev), batch["occ"].to(dev)
        transmat = batch["transmat"].to(dev) if "transmat" in batch else None
        pred = self.model(img, points, transmat)
        return pred, (self.calc_loss(pred, [occ_gt, sdf_gt]) if calc_loss else [])

    @torch.no_grad()
    def predict_grid(self, img, transmat=None, res=None, shard=True, refine=None, band=None, level=0.0):
        """SDF on the regular res^3 grid over [-0.5,0.5]^3 (reference executors.py:191-231) ->
        float32 tensor [res,res,res] on the device, already divided by sdf_scale.

        The grid is generated on the device chunk by chunk (no host->device point copies, no
        per-chunk .cpu()); with torch.distributed initialised and shard=True the query axis is split
        over the ranks and all-gathered.

        refine=s (2, 4 or 8): the coarse-to-fine grid of refine.predict_grid_refined -- the network is queried on the
        stride-s lattice and at the fine points of the bricks near the iso-level `level` (band: refine.default_band
        when None); the other points are interpolated.  Queried points equal the dense grid's bit for bit; the
        counts land in self.last_grid_stats.  refine=None: every point is queried."""
        if refine:
            return self._predict_grid_refined(img, transmat, res, shard, refine, band, level)
        net = _unwrap(self.model)
        dev = img.device
        res = res or self.query_res
        feat_l2, vox_feat, transmat, _, occ = net.encode(img, transmat)
        self.last_transmat = transmat
        total = res ** 3
        rank, world = parallel.world_info() if shard else (0, 1)
        if world > 1:        # every rank samples rank 0's maps: sharded == unsharded bit for bit (parallel.py)
            parallel.broadcast_from_rank0(list(feat_l2) + list(vox_feat) + [transmat, occ])
        begin, end = parallel.shard_range(total, rank, world)
        out = torch.empty((end - begin,), dtype=torch.float32, device=dev)
        # --test_pointnum bounds the reference's per-chunk memory (executors.py:199-231).  Here the query's memory does
        # not depend on the call size (the library cuts a call into row chunks of its fixed workspace, bit-identical),
        # and a 65 536-point call is dominated by its ~20 launches and the Python dispatch: calls of at least 2^20
        # points (256^3 grid: 111.6 -> 142 M points/s in fp16, 69 -> 78 M in bf16x3)
        step = max(int(self.test_pointnum), 1 << 20)
        # one decision for the whole grid (every call and every rank of a sharded grid then computes the same bits): with
        # at least 4 x 137^2 points on the image, fc_0's perceptual block is applied to the map once (hotpath.sdf_query)
        ms = net.percep_pooling.map_size
        project = total >= 4 * ms * ms
        for s in range(begin, end, step):
            e = min(s + step, end)
            pts = utils.grid_points_on_device(-0.5, 0.5, res, dev, s, e).unsqueeze(0)
            # (raster order: consecutive grid points are neighbours already, the forward skips its point sort)
            out[s - begin:e - begin] = net.query_sdf(pts, feat_l2, vox_feat, transmat, ordered_points=True,
                                                     project_percep=project)[0]
        if world > 1:
            out = parallel.gather_ragged_points(out, total)
        return (out / self.sdf_scale).view(res, res, res), occ, vox_feat

    def _predict_grid_refined(self, img, transmat, res, shard, stride, band, level):
        net = _unwrap(self.model)
        dev = img.device
        res = res or self.query_res
        feat_l2, vox_feat, transmat, _, occ = net.encode(img, transmat)
        self.last_transmat = transmat
        rank, world = parallel.world_info() if shard else (0, 1)
        if world > 1:        # as the dense grid: every rank samples rank 0's maps
            parallel.broadcast_from_rank0(list(feat_l2) + list(vox_feat) + [transmat, occ])
        ms = net.percep_pooling.map_size
        project = res ** 3 >= 4 * ms * ms             # the dense grid's decision: every queried point gets its bits

        def query(pts):
            # the dense grid's per-point arithmetic, the division by sdf_scale included (the same torch expression)
            return net.query_sdf(pts, feat_l2, vox_feat, transmat, ordered_points=True,
                                 project_percep=project)[0] / self.sdf_scale

        vol, self.last_grid_stats = RF.predict_grid_refined(query, res, int(stride), band=band, level=level,
                                                            device=dev, step=max(int(self.test_pointnum), 1 << 20),
                                                            shard=shard)
        return vol, occ, vox_feat

    def test(self, batch, eval_pred=False):
        img = batch["rgb_image"].to(self._device())
        transmat = batch["transmat"].to(self._device()) if "transmat" in batch else None
        volume, occ, vox_feat = (self.predict_grid(img, transmat, refine=self.refine_stride, band=self.refine_band)
                                 if self.refine_stride else self.predict_grid(img, transmat))
        # marching cubes on the device, where the volume lies (mesh.marching_cubes: mcubes' surface of -volume at 0)
        pred_mesh = mesh.Mesh(*self.filter_mesh(*mesh.marching_cubes(volume, 0.0, -0.5, 0.5)))
        score = self.eval(pred_mesh, batch.get("gt_mesh")) if eval_pred else {}
        return [pred_mesh, occ, vox_feat[0].squeeze(1)], score

    def filter_mesh(self, verts, faces):
        """The mesh as marching_cubes left it on the device, first without the components --mesh_components /
        --mesh_min_faces drop (components.keep_components on the full-resolution mesh; its info lands in
        self.last_components), then simplified on the --mesh_simplify grid (simplify.simplify; its info lands in
        self.last_simplify).  With all three at 0 the tensors come back untouched."""
        if self.mesh_components or self.mesh_min_faces:
            verts, faces, self.last_components = components.keep_components(
                verts, faces, keep=self.mesh_components or "all", min_faces=self.mesh_min_faces)
        if self.mesh_simplify:
            verts, faces, self.last_simplify = simplify.simplify(verts, faces, self.mesh_simplify, self.bb_min,
                                                                 self.bb_max)
        return verts, faces

    def eval(self, pred, gt):
        """eval_util.py:eval_mesh of the predicted mesh against the ground truth (a Mesh or a path to one), on the
        executor's device -> the reference's dict of floats ({} for a prediction of fewer than 10 vertices)."""
        if gt is None:
            raise ValueError("LIST.eval: no ground-truth mesh (the batch carries no 'gt_mesh')")
        return evaluate.eval_mesh(pred, gt, self.bb_min, self.bb_max, device=self._device())

    def render_views(self, batch, pred, which=None):
        """Pictures of the predicted mesh (pred: test()'s list, or the Mesh) -> {name: uint8 [S,S,3]}, S = --render_size.
        "view": the mesh from the camera predict_grid used (self.last_transmat; else the batch's 'transmat'), head-light
        grey at VIEW_ALPHA over the input image resized to S x S -- where the network sampled the image, is the shape on
        the object?  "x", "y", "z": orthographic head-light views along array axis 0, 1, 2 of the volume.  which: 'view',
        'canonical' or 'both' (default: --render_pred, 'both' when that is 'none').  Without a camera there is no "view";
        a mesh without a valid face gives the background."""
        m = pred[0] if isinstance(pred, (list, tuple)) else pred
        which = which or (self.render_pred if self.render_pred != "none" else "both")
        S = self.render_size
        out = {}
        tm = self.last_transmat if self.last_transmat is not None else batch.get("transmat")
        if RENDER_VIEWS[which][0] and tm is not None:
            if hasattr(tm, "detach"):
                tm = tm.detach().float().cpu().numpy()
            net = _unwrap(self.model)
            map_size = getattr(getattr(net, "percep_pooling", None), "map_size", 137)
            cam = render.Camera.from_transmat(np.asarray(tm, dtype=np.float32).reshape(-1, 4, 3)[0], map_size)
            out["view"] = m.render(cam, S, S, "lambert", self._input_image(batch, S), VIEW_ALPHA)
        if RENDER_VIEWS[which][1]:
            for axis, name in enumerate("xyz"):
                cam = render.Camera.orthographic(axis, S, S, self.bb_min, self.bb_max)
                out[name] = m.render(cam, S, S, "lambert")
        return out

    @staticmethod
    def _input_image(batch, S):
        """The batch's first 'rgb_image' ([B,3,H,W] or [3,H,W], values in [0,1]) as uint8 [S,S,3]; None without one."""
        img = batch.get("rgb_image")
        if img is None:
            return None
        img = torch.as_tensor(img).detach().float().cpu()
        img = img[0] if img.dim() == 4 else img
        if img.shape[-2:] != (S, S):
            img = torch.nn.functional.interpolate(img[None], size=(S, S), mode="bilinear", align_corners=False)[0]
        return (img.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()

    def save(self, batch, pred, fname):
        pred[0].export(fname + "_pred.obj")
        if self.render_pred != "none":
            for name, img in self.render_views(batch, pred).items():
                render.save_png(f"{fname}_pred_{name}.png", img)
