"""Objective scores used by AcousticModelTrainer.benchmark (reference: idiaptts/src/Metrics.py):
mel-cepstral distortion (nnmnkwii melcd formula 10/ln10 * sqrt(2) * mean_t ||dc||_2, c_0
excluded), F0 RMSE on frames voiced in the original, voicing decision error, band-aperiodicity
distortion. Tiny host-side numpy; needed by the parity harness, not a kernel."""
import math

import numpy as np


class Metrics(object):
    MCD = "MCD"
    F0_RMSE = "F0 RMSE"
    VDE = "VDE"
    BAP_distortion = "BAP distortion"
    Dur_RMSE = "Dur RMSE"
    Dur_pearson = "Dur pearson"

    @staticmethod
    def rmse(org, output, axis=None):
        """sqrt(sum of squared errors / number of ROWS) (reference :165-171: with axis=None the sum
        runs over all elements but the divisor stays the row count)."""
        mse = (org - output) ** 2
        return np.sqrt(mse.sum(axis=axis) / len(mse))

    @staticmethod
    def pearson(org, output):
        """Pearson correlation per column (reference :173-175, scipy.stats.pearsonr)."""
        o = org - org.mean(axis=0)
        p = output - output.mean(axis=0)
        return (o * p).sum(axis=0) / np.sqrt((o * o).sum(axis=0) * (p * p).sum(axis=0))

    @staticmethod
    def melcd(x, y):
        return float(10.0 / np.log(10) * np.sqrt(2.0) * np.sqrt(((x - y) ** 2).sum(-1)).mean())

    @staticmethod
    def mcd_k(org_cep, output_cep, k=None, start_bin=1):
        org = org_cep[:len(output_cep)]
        return Metrics.melcd(output_cep[:, start_bin:k], org[:, start_bin:k])

    @staticmethod
    def f0_rmse(org_lf0, org_vuv, output_lf0):
        org_f0 = np.exp(org_lf0.squeeze())[:len(output_lf0)]
        org_vuv = org_vuv[:len(output_lf0)]
        f0_mse = (org_f0 - np.exp(output_lf0)) ** 2
        return math.sqrt((f0_mse * org_vuv).sum() / org_vuv.sum())

    @staticmethod
    def voicing_decision_error(org_vuv, output_vuv):
        return (org_vuv[:len(output_vuv)] != output_vuv).sum() / len(output_vuv)

    @staticmethod
    def aperiodicity_distortion(org_bap, output_bap):
        org_bap = org_bap[:len(output_bap)]
        if output_bap.ndim > 1 and output_bap.shape[1] > 1:
            return Metrics.mcd_k(org_bap, output_bap)
        return math.sqrt(((org_bap - output_bap) ** 2).mean()) * (10.0 / np.log(10) * np.sqrt(2.0))

    @staticmethod
    def get_metrics(org, output):
        """org / output: (coded_sp, lf0, vuv, bap) tuples -> [MCD, F0 RMSE, VDE, BAP distortion]."""
        o_sp, o_lf0, o_vuv, o_bap = org
        p_sp, p_lf0, p_vuv, p_bap = output
        return [Metrics.mcd_k(o_sp, p_sp), Metrics.f0_rmse(o_lf0, o_vuv, p_lf0),
                Metrics.voicing_decision_error(o_vuv, p_vuv),
                Metrics.aperiodicity_distortion(o_bap, p_bap)]

    # ---- the same scores along a dynamic-time-warping path (not in the reference): for outputs whose length is not
    # the original's (predicted durations, another hop, re-analysed audio) frame t of one is not frame t of the other.
    # The two coded spectra (bin 0 left out, as mcd_k does) are aligned on the GPU (ops.dtw_align, csrc/dtw.hip) and
    # every score is get_metrics' formula over the aligned pairs (i, j) instead of over t.
    MELCD_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)

    @staticmethod
    def _device_f64(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to("cuda")

    @staticmethod
    def dtw_path(org_cep, output_cep, start_bin=1, k=None, band=None):
        """(path int32 [L, 2] of (original frame, output frame) pairs, cost) of the DTW of org_cep[:, start_bin:k]
        against output_cep[:, start_bin:k]; the MCD along it is MELCD_CONST * cost / L."""
        from idiaptts_amd import ops
        x = Metrics._device_f64(np.asarray(org_cep)[:, start_bin:k])
        y = Metrics._device_f64(np.asarray(output_cep)[:, start_bin:k])
        cost, length, path = ops.dtw_align([x], None, [y], None, band=band)
        cost = float(cost[0].item())
        if not math.isfinite(cost):
            raise ValueError("dtw_path: band = {} does not connect the two sequences' ends ({} x {} frames)".format(
                band, len(org_cep), len(output_cep)))
        return path[0, :int(length[0].item())].cpu().numpy(), cost

    @staticmethod
    def get_metrics_dtw_batch(orgs, outputs, band=None):
        """[n, 4] array of [MCD, F0 RMSE, VDE, BAP distortion] for n (org, output) pairs of (coded_sp, lf0, vuv, bap)
        tuples, each score taken along the pair's DTW path; one ops.dtw_align call aligns all pairs, the gathers along
        the paths are float64 torch ops on the device."""
        import torch
        from idiaptts_amd import ops
        if len(orgs) != len(outputs):
            raise ValueError("get_metrics_dtw_batch: {} originals, {} outputs".format(len(orgs), len(outputs)))
        dev = Metrics._device_f64
        xs = [dev(np.asarray(o[0])[:, 1:]) for o in orgs]
        ys = [dev(np.asarray(p[0])[:, 1:]) for p in outputs]
        cost, length, path = ops.dtw_align(xs, None, ys, None, band=band)
        cost_h, length_h = cost.cpu().numpy(), length.cpu().numpy()
        scores = np.empty((len(orgs), 4), dtype=np.float64)
        for n, (org, out) in enumerate(zip(orgs, outputs)):
            if not math.isfinite(cost_h[n]):
                raise ValueError("get_metrics_dtw_batch: band = {} does not connect the ends of pair {} "
                                 "({} x {} frames)".format(band, n, len(org[0]), len(out[0])))
            L = int(length_h[n])
            pi, pj = path[n, :L, 0].long(), path[n, :L, 1].long()
            o_lf0, o_vuv = dev(np.asarray(org[1]).reshape(-1)), dev(np.asarray(org[2]).reshape(-1))
            p_lf0, p_vuv = dev(np.asarray(out[1]).reshape(-1)), dev(np.asarray(out[2]).reshape(-1))
            o_bap, p_bap = np.asarray(org[3]), np.asarray(out[3])
            v = o_vuv[pi]
            f0_se = (torch.exp(o_lf0[pi]) - torch.exp(p_lf0[pj])) ** 2
            f0_rmse = torch.sqrt((f0_se * v).sum() / v.sum())                 # NaN without a voiced original frame
            vde = (v != p_vuv[pj]).sum().to(torch.float64) / L
            if p_bap.ndim > 1 and p_bap.shape[1] > 1:                         # multi-band: the mcd_k form, band 0 dropped
                diff = dev(o_bap[:, 1:])[pi] - dev(p_bap[:, 1:])[pj]
                bap = Metrics.MELCD_CONST * torch.sqrt((diff ** 2).sum(-1)).mean()
            else:
                diff = dev(o_bap.reshape(-1))[pi] - dev(p_bap.reshape(-1))[pj]
                bap = Metrics.MELCD_CONST * torch.sqrt((diff ** 2).mean())
            scores[n] = [Metrics.MELCD_CONST * cost_h[n] / L, float(f0_rmse.item()), float(vde.item()),
                         float(bap.item())]
        return scores

    @staticmethod
    def get_metrics_dtw(org, output, band=None):
        """get_metrics along the DTW path of the two coded spectra: [MCD, F0 RMSE, VDE, BAP distortion]."""
        return [float(v) for v in Metrics.get_metrics_dtw_batch([org], [output], band=band)[0]]

    @staticmethod
    def compare_wav_lists(org_files, synth_files, hparams, band=None):
        """[n, 4] DTW scores of n synthesised wav files against n recordings: both lists go through the batched WORLD
        analysis and mel-cepstrum gen_data uses (hparams.synth_fs, num_coded_sps, frame_size_ms, preemphasis), then
        through get_metrics_dtw_batch.  A file whose sampling rate is not synth_fs is refused by name."""
        from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
        from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
        if len(org_files) != len(synth_files):
            raise ValueError("compare_wav_lists: {} original files, {} synthesised files".format(
                len(org_files), len(synth_files)))
        fs = int(hparams.synth_fs)
        preemphasis = getattr(hparams, "preemphasis", 0.0)          # (not among create_hparams' defaults; 0 as the Synthesiser)
        raws = []
        for name in list(org_files) + list(synth_files):
            raw, file_fs = AudioProcessing.get_raw(name, preemphasis)
            if int(file_fs) != fs:
                raise ValueError("compare_wav_lists: {} is sampled at {} Hz, hparams.synth_fs is {} Hz".format(
                    name, file_fs, fs))
            raws.append(raw)
        feats = WorldFeatLabelGen.extract_features_batch(raws, fs, hop_size_ms=hparams.frame_size_ms,
                                                         num_coded_sps=hparams.num_coded_sps)
        n = len(org_files)
        return Metrics.get_metrics_dtw_batch(feats[:n], feats[n:], band=band)
