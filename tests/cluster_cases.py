"""What tests/test_gpu_clusters.py and tests/test_gpu_cluster_mirror.py hold a device result to: the
restatement (tests/cluster_restatement.py) and the bounds stated in tests/test_gpu_clusters.py.  Test
infrastructure only."""
import math

import numpy as np

import cluster_restatement as R

BOUND = 64.0 * 2.0 ** -53


def compare(got, want, max_clusters=8):
    """got = (header, records, labels) as Clusterer.fetch_raw() and labels() give them (any objects
    with those fields); want = cluster_restatement.cluster() of the same input."""
    header, records, labels = got
    assert np.array_equal(labels, want["labels"])
    wh = want["header"]
    assert (header.n, header.n_left_out, header.n_bins, header.n_clusters) == \
        (wh["n"], wh["n_left_out"], wh["n_bins"], wh["n_clusters"])
    assert abs(header.w_total - wh["w_total"]) <= BOUND * wh["w_total"]
    assert len(records) == min(max_clusters, wh["n_clusters"]) == len(want["records"])
    assert int(labels[labels != R.LEFT_OUT].size) + header.n_left_out == header.n
    for g, w in zip(records, want["records"]):
        q = g.mass * 2.0 ** 40
        assert q == math.floor(q) and (g.label, g.count, int(q)) == (w["label"], w["count"], w["Q"])
        a = w["abs"]
        print("cluster %d: count %d, W %.17g (off %.2e), mean (%.17g, %.17g, %.17g)" %
              (g.label, g.count, g.weight, abs(g.weight - w["W"]), g.mean_x, g.mean_y, g.mean_theta))
        assert abs(g.weight - w["W"]) <= BOUND * a["W"]
        if w["W"] == 0.0:
            continue                                  # (statistics over no weight are not numbers, on both sides)
        for name, got_v, want_v, terms in (("mean_x", g.mean_x, w["mx"], a["x"]), ("mean_y", g.mean_y, w["my"], a["y"])):
            assert abs(got_v - want_v) <= BOUND * terms / w["W"], (name, got_v, want_v, terms)
        # the second pass: the centred terms round the means the device reports (held to the fsum
        # means just above and below), summed by fsum
        m, m_abs = R.centred_moments(want["poses"], want["weights"], w["members"], w["W"], g.mean_x, g.mean_y, g.mean_theta)
        for name, got_v, short in (("cxx", g.cxx, "xx"), ("cxy", g.cxy, "xy"), ("cyy", g.cyy, "yy"), ("vt", g.var_theta, "tt")):
            assert abs(got_v - m[name]) <= BOUND * m_abs[short] / w["W"], (name, got_v, m[name], m_abs[short])
            # and the restatement's own moments, round its own means, differ from them by no more
            # than moving the centre by the means' bound moves them
            assert abs(m[name] - w[name]) <= 1e-9 * (m_abs[short] + a[short]) / w["W"] + 1e-24, (name, m[name], w[name])
        if w["resultant"] >= 0.1:
            d = abs(float(R.normalise_angle(g.mean_theta - w["mt"])))
            assert d <= 1e-12, (g.mean_theta, w["mt"])
