"""The jax.random draws of ONE update call, built on the host from the call's keys: the `noise` dict AgentCore._noise takes.

DrQAgent / SACAgent (whole batch, any number of critic updates per call) and the learners of serl_amd/parallel.py (one critic
update per call, a rank's rows of the global batch) both build it here; the C side has one mechanism too (agent.hip PhaseNoise /
draw_noise).  What a call draws (sac.py:118-157,197-227): per critic update the next-action normals and the policy encoder's
Dropout masks from k_next_action[i] and the REDQ subsample from k_subsample[i]; for the actor + temperature update the
normals from k_sample / k_temp and the masks from k_policy / k_temp.  A camera's Dropout key is flax's make_rng at the layer's
scope path (jaxrng.flax_make_rng); only the frozen-trunk encoder has Dropout (the SmallEncoder pools with "avg").
An agent with MLP Dropout (mlp.py:27-28; AgentCore.critic_dropout / policy_dropout) draws two more masks in each of its six MLP
evaluations (_lib_agent.MLP_SITES): the policy's from the rng of that policy forward, the critic's from k_q_target / k_q_online /
k_q_actor (jaxrng.UpdateKeys), each layer's key being flax's make_rng at jaxrng.mlp_dropout_path."""
from __future__ import annotations

import numpy as np

from . import jaxrng as J
from ._lib_agent import MLP_CRITIC_LOSS_SITES, MLP_SITE_NETWORK


class CallNoise:
    def __init__(self, core, image_keys, last_draws: dict, ensemble: int = 10):
        """core: supplies cfg, device and _stream(); a duck-typed core without cfg (CPU tests) gets REDQ indices only: 2 of
        `ensemble`.  last_draws: the caller's record of what its last call drew (the REDQ indices are written into it)."""
        self.core, self.image_keys, self.last_draws, self.ensemble = core, tuple(image_keys or ()), last_draws, ensemble
        self.bufs = {}       # {local rows: {name: device tensor}} of the "tensors" form, for the last row count used
        # scope path of an MLP Dropout layer, (network, layer) -> names from the root: data, so that a parity run against another
        # module tree can state its own
        self.mlp_dropout_path = J.mlp_dropout_path

    def mlp_rates(self):
        """{"critic": rate, "policy": rate} of the core's MLP Dropout (zeros for a core without the attributes)"""
        return {"critic": float(getattr(self.core, "critic_dropout", 0.0)), "policy": float(getattr(self.core, "policy_dropout", 0.0))}

    def mlp_site_keys(self, keys: J.UpdateKeys, want_critic: bool, want_actor: bool):
        """{site: rng of that forward -- a list per critic update for the critic-loss sites} for the sites whose network drops"""
        rates, out = self.mlp_rates(), {}
        if want_critic:
            out.update(pi_next=keys.k_next_action)
            if rates["critic"] > 0:
                out.update(q_target=keys.k_q_target, q_online=keys.k_q_online)
        if want_actor:
            out.update(pi=keys.k_policy, pi_temp=keys.k_temp)
            if rates["critic"] > 0:
                out.update(q_actor=keys.k_q_actor)
        return {site: k for site, k in out.items() if rates[MLP_SITE_NETWORK[site]] > 0}

    def _layer_keys(self, site, rng):
        return np.stack([J.flax_make_rng(rng, self.mlp_dropout_path(MLP_SITE_NETWORK[site], l), 1) for l in (0, 1)])

    def _buffers(self, rows, A, D, n_cam):
        if rows not in self.bufs:
            import torch
            dev = self.core.device
            nb = {k: torch.empty((rows, A), dtype=torch.float32, device=dev) for k in ("eps_next", "eps_pi", "eps_temp")}
            if n_cam:
                nb.update({k: torch.empty((n_cam, rows, D), dtype=torch.uint8, device=dev) for k in ("mask_next", "mask_obs_pi", "mask_next_temp")})
            self.bufs = {rows: nb}
        return self.bufs[rows]

    def build(self, keys: J.UpdateKeys, rows: int, form: str = "keys", want_critic: bool = True, want_actor: bool = True,
              shard=None, device_draws: bool = True):
        """rows: the local batch.  form "keys": the consuming kernels draw in place from the call's keys (key_eps_next uint32[update][2],
        key_mask_next uint32[update][camera][2]; a sharded core draws its rows of the global arrays itself, serl_agent_set_shard).
        form "tensors": one serl_jax_fill launch writes the draws -- critic update i into rows [i*mb, (i+1)*mb) from key i, in
        the reference's shapes ((mb, A) normals, one (mb, 4096) mask per camera).  shard = (lo, global_rows): the local rows are
        rows [lo, lo + rows) of the global arrays (one critic update per call).  device_draws False (noise hashed inside the
        kernels): only the REDQ indices, which always come from the key schedule; None when the call has none."""
        cfg = getattr(self.core, "cfg", None)
        want_critic, want_actor = want_critic and keys.n_critic > 0, want_actor and keys.has_actor_temp
        noise = {}
        m, ensemble = (2, self.ensemble) if cfg is None else (int(cfg.critic_subsample_size), cfg.ensemble)
        if want_critic and m > 0:       # (critic_subsample_size None: the minimum runs over the whole ensemble, no draw)
            noise["redq_idx"] = np.stack([J.randint(k, m, 0, ensemble) for k in keys.k_subsample]).astype(np.int32)
            self.last_draws["redq_idx"] = noise["redq_idx"].copy()
        if not device_draws:
            return noise or None
        cams = self.image_keys[:cfg.n_cam] if cfg.encoder_type == 0 else ()
        cam_keys = lambda k: [J.flax_make_rng(k, J.dropout_path(cam), 1) for cam in cams]  # noqa: E731
        mlp = self.mlp_site_keys(keys, want_critic, want_actor)
        if form == "keys":
            for site, k in mlp.items():      # [update][layer][2] for the critic-loss sites, [layer][2] for the others
                noise["drop_key_" + site] = (np.stack([self._layer_keys(site, ki) for ki in k]) if site in MLP_CRITIC_LOSS_SITES
                                             else self._layer_keys(site, k))
            if want_critic:
                noise["key_eps_next"] = np.stack(keys.k_next_action)
                if cams:
                    noise["key_mask_next"] = np.stack([cam_keys(k) for k in keys.k_next_action])
            if want_actor:
                noise["key_eps_pi"], noise["key_eps_temp"] = keys.k_sample, keys.k_temp
                if cams:
                    noise["key_mask_obs_pi"], noise["key_mask_next_temp"] = np.stack(cam_keys(keys.k_policy)), np.stack(cam_keys(keys.k_temp))
            return noise
        assert form == "tensors", form
        assert shard is None or keys.n_critic <= 1, "a sharded call makes one critic update"
        lo = 0 if shard is None else shard[0]
        A, D, keep = cfg.act_dim, 512 * cfg.sle_features, 1.0 - float(cfg.dropout)
        nb, jobs = self._buffers(rows, A, D, len(cams)), []

        def draws(eps, eps_key, mask, mask_key, row0=0, n=rows):
            """local rows [row0, row0 + n) <- rows [lo, lo + n) of the g-row arrays jax.random draws from the keys"""
            g = n if shard is None else shard[1]
            jobs.append(J.job(J.NORMAL, eps_key, g * A, nb[eps].data_ptr() + row0 * A * 4, first=lo * A, count=n * A))
            noise[eps] = nb[eps]
            for ci, k in enumerate(cam_keys(mask_key)):
                jobs.append(J.job(J.BERNOULLI_U8, k, g * D, nb[mask].data_ptr() + (ci * rows + row0) * D, first=lo * D, count=n * D, p=keep))
                noise[mask] = nb[mask]

        def mlp_draws(site, rng, row0=0, n=rows):
            """the site's two keep-masks u8[2, rows, hidden]: local rows [row0, row0 + n) <- rows [lo, lo + n) of each layer's draw"""
            name, h = "drop_mask_" + site, int(cfg.hidden)
            if name not in nb:
                import torch
                nb[name] = torch.empty((2, rows, h), dtype=torch.uint8, device=self.core.device)
            g = n if shard is None else shard[1]
            p = 1.0 - self.mlp_rates()[MLP_SITE_NETWORK[site]]
            for l, k in enumerate(self._layer_keys(site, rng)):
                jobs.append(J.job(J.BERNOULLI_U8, k, g * h, nb[name].data_ptr() + (l * rows + row0) * h, first=lo * h, count=n * h, p=p))
            noise[name] = nb[name]

        if want_critic:
            mb = rows // keys.n_critic
            for i, k in enumerate(keys.k_next_action):
                draws("eps_next", k, "mask_next", k, i * mb, mb)
                for site in MLP_CRITIC_LOSS_SITES:
                    if site in mlp:
                        mlp_draws(site, mlp[site][i], i * mb, mb)
        for site, k in mlp.items():
            if site not in MLP_CRITIC_LOSS_SITES:
                mlp_draws(site, k)
        if want_actor:
            draws("eps_pi", keys.k_sample, "mask_obs_pi", keys.k_policy)
            draws("eps_temp", keys.k_temp, "mask_next_temp", keys.k_temp)
        J.fill(cfg.device, jobs, self.core._stream())
        return noise
