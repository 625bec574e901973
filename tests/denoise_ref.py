"""The denoiser's contract (include/ort.h, ort_denoise) restated in numpy float32, written from the header's text and from
nothing else: whole planes at a time, a tap being a shifted view of a plane.  Every arithmetic step is one numpy float32
operation, so it rounds once, as the contract says; numpy fuses nothing.  The tests compare the library's and the host
simulator's frames with this one bit for bit (NaN by position)."""
import numpy as np

F = np.float32
K5 = (F(0.375), F(0.25), F(0.0625))
K3 = (F(0.5), F(0.25))


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def fall(x):
    r = F(1.0) / (F(1.0) + x)
    r = r * r
    r = r * r
    return r


def _shift(a, ox, oy):
    """-> (b, inside) with b[y, x] = a[y + oy, x + ox] where that lies inside the frame (0 elsewhere)"""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    if abs(ox) >= w or abs(oy) >= h:
        return b, inside
    ys, yd = (slice(oy, h), slice(0, h - oy)) if oy >= 0 else (slice(0, h + oy), slice(-oy, h))
    xs, xd = (slice(ox, w), slice(0, w - ox)) if ox >= 0 else (slice(0, w + ox), slice(-ox, w))
    b[yd, xd] = a[ys, xs]
    inside[yd, xd] = True
    return b, inside


def denoise_frame(rgb, m2, count, albedo, normal, depth, iterations, normal_squarings, sigma_l, sigma_z):
    """one frame: (H, W[, 3]) planes -> (H, W, 3) float32"""
    rgb, m2, albedo, normal, depth = (np.asarray(a, "<f4") for a in (rgb, m2, albedo, normal, depth))
    count = np.asarray(count, "<u4")
    sigma_l, sigma_z = F(sigma_l), F(sigma_z)
    with np.errstate(all="ignore"):
        fn = count.astype(F)
        a = np.where(albedo > F(1e-3), albedo, F(1e-3)).astype(F)
        c = rgb / a
        Y = lum(rgb)
        v = m2 / fn - Y * Y
        v = np.where(v < 0, F(0), v)
        vm = np.where(count > 1, v / (fn - F(1.0)), Y * Y)
        la = lum(a)
        var = (vm / (la * la)).astype(F)
        usable = count >= 1
        for plane in (rgb, albedo, normal, c):
            usable &= np.isfinite(plane).all(axis=-1)
        for plane in (m2, depth, var):
            usable &= np.isfinite(plane)

        sl2, sz2 = sigma_l * sigma_l, sigma_z * sigma_z
        for j in range(iterations):
            s = 1 << j
            G = np.zeros(var.shape, F)
            GW = np.zeros(var.shape, F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, inside = _shift(var, dx, dy)
                    uq, _ = _shift(usable, dx, dy)
                    take = inside & uq
                    w3 = K3[abs(dx)] * K3[abs(dy)]
                    G = np.where(take, G + w3 * vq, G)
                    GW = np.where(take, GW + w3, GW)
            g = G / GW
            lp = lum(c)
            den = sl2 * g + F(1e-10)
            S = np.zeros(c.shape, F)
            V = np.zeros(var.shape, F)
            W = np.zeros(var.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, inside = _shift(c, s * dx, s * dy)
                    vq, _ = _shift(var, s * dx, s * dy)
                    uq, _ = _shift(usable, s * dx, s * dy)
                    take = inside & uq
                    h = K5[abs(dx)] * K5[abs(dy)]
                    if dx == 0 and dy == 0:
                        w = np.full(var.shape, h, F)
                    else:
                        nq, _ = _shift(normal, s * dx, s * dy)
                        zq, _ = _shift(depth, s * dx, s * dy)
                        d = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                        wn = np.where(d > 0, d, F(0))
                        for _ in range(normal_squarings):
                            wn = wn * wn
                        dz = depth - zq
                        zm = np.maximum(np.abs(depth), np.abs(zq))
                        xz = (dz * dz) / (((zm * zm) * F(s * s * (dx * dx + dy * dy))) * sz2)
                        dl = lp - lum(cq)
                        xl = (dl * dl) / den
                        w = ((h * wn) * fall(xz)) * fall(xl)
                        w = np.where(np.isfinite(w), w, F(0))
                    S = np.where(take[..., None], S + w[..., None] * cq, S)
                    V = np.where(take, V + (w * w) * vq, V)
                    W = np.where(take, W + w, W)
            c = np.where(usable[..., None], S / W[..., None], c).astype(F)
            var = np.where(usable, V / (W * W), var).astype(F)
        out = (c * a).astype("<f4")
    out[~usable] = rgb[~usable]
    return out


def denoise(rgb, m2, count, albedo, normal, depth, iterations=5, normal_squarings=5, sigma_l=4.0, sigma_z=0.05):
    """(H, W[, 3]) planes, or (V, H, W[, 3]): every frame on its own"""
    if np.ndim(count) == 2:
        return denoise_frame(rgb, m2, count, albedo, normal, depth, iterations, normal_squarings, sigma_l, sigma_z)
    return np.stack([denoise_frame(rgb[v], m2[v], count[v], albedo[v], normal[v], depth[v], iterations, normal_squarings, sigma_l, sigma_z)
                     for v in range(len(count))])
