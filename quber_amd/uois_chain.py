"""The UOIS-Net-3D chain on the device, stage by stage: Depth Seeding Network -> Gaussian mean shift + IMP -> crops, Region Refinement
Network, paste (-> final close).  ``MaskRefinerPredictor`` runs the three stages at the points of its pass where their inputs are ready
(the network before the pass, the clustering and the refinement inside it); ``uois_chain`` runs them back to back on a frame engine
without a refiner network, which is what ``quber_amd.eval.base_model.UOISNet`` is.  One implementation of each stage for both."""
import numpy as np
import torch


def mask_rows(cluster, h, w):
    """rows of the mask tensor per frame under a GaussianMeanShift: a label per seed, each with min_pixels pixels of the frame"""
    return min(cluster.num_seeds, 254, max(h * w // max(cluster.min_pixels, 1), 1))


def seed_stage(seeding, cluster, x, camera=None):
    """x: xyz f32 [B,3,H,W] on the device, or with camera= (a quber_amd.camera.Camera) z f32 [B,H,W] -> ((votes, fg, first, draws) for
    Engine.gms, all on the device; the class map u8 [B,H,W]; the class counts i64 [B,3] on the host).  One D2H of 3 B + 1 integers: the
    draw of a frame's first seed needs its foreground count."""
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    dsn = seeding.engine_for(H, W, B, x.device)
    votes, on, cls = dsn.seed(x) if camera is None else dsn.seed(z=x, camera=camera)
    tally = torch.stack([(cls == k).sum((1, 2)) for k in range(3)], 1)
    host = torch.cat([tally.reshape(-1), torch.isfinite(votes).all().to(torch.int64)[None]]).cpu().numpy()
    if not host[-1]:
        raise ValueError("seeding: the centre votes are not finite (xyz must be finite, or NaN where there is no depth)")
    tally = host[:-1].reshape(B, 3)
    first, draws = cluster.draws([cluster.n_sub(int(n)) for n in tally[:, 2]])
    dev = lambda a: torch.from_numpy(a).to(x.device)
    return (votes, on, dev(first), dev(draws.view(np.int32))), cls, tally


def cluster_stage(eng, cluster, cluster_in, n_rows):
    """cluster_in = (votes f32 [B,3,H,W], fg u8 [B,H,W], first i32 [B], draws i32 [B,S]) -> what Engine.gms returns"""
    return eng.gms(*cluster_in, cluster, n_rows)


def region_stage(eng, region, bgr, cl, n_rows, z):
    """the clustered masks of bgr's frames cropped, refined and painted back (RegionRefinement.refine).  One small read-back, the
    per-frame cluster counts, builds the slot list.  -> what refine returns, plus "counts"."""
    B = bgr.shape[0]
    counts = cl["report"][:B, 0].cpu().numpy()
    rg = region.refine(eng, bgr, cl["ids"], n_rows, counts, z)
    rg["counts"] = counts
    return rg


def uois_chain(eng, seeding, cluster, region, bgr, x, camera=None):
    """The whole chain on frame engine `eng`: bgr u8 [B,H,W,3], x = xyz f32 [B,3,H,W] or (camera=) z f32 [B,H,W], on the device ->
    {"cluster": Engine.gms's dict, "region": RegionRefinement.refine's dict or None, "classes": u8 [B,H,W], "tally": i64 [B,3]}."""
    n_rows = mask_rows(cluster, eng.H, eng.W)
    cluster_in, cls, tally = seed_stage(seeding, cluster, x, camera)
    cl = cluster_stage(eng, cluster, cluster_in, n_rows)
    rg = None
    if region is not None:
        rg = region_stage(eng, region, bgr, cl, n_rows, x if camera is not None else x[:, 2].contiguous())
    return {"cluster": cl, "region": rg, "classes": cls, "tally": tally}
