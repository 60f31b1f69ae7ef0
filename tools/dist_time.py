import os, sys, numpy as np, torch
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT','/root/repo'))
from numbotics_amd.physics import World
from numbotics_amd.scenes import build_scene, sample_q
World()
SCENE = sys.argv[1] if len(sys.argv) > 1 else 'c2'
arm, chain, obs = build_scene(SCENE)
sm, dev = arm._scene_device()
B = 200000 if SCENE == 'c2' else 50000
q = torch.from_numpy(sample_q(chain, B, seed=1)).cuda()
def t(fn, n=5):
    fn(); torch.cuda.synchronize()
    e0,e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)/n
print('scene', SCENE, 'pairs', sm.n_pairs, 'hulls', sm.n_hulls)
Bv = 1000000
qv = torch.from_numpy(sample_q(chain, Bv, seed=1)).cuda()
for thr in (0.0, 1e-6):
    print('validity thr %g: ms %.3f for %d -> %.3e cfg/s' % (thr, (ms := t(lambda: dev.validity(qv, thr, packed=True), 10)), Bv, Bv / ms * 1e3))
print('closest ms %.3f for %d -> %.3e cfg/s'%((ms:=t(lambda: dev.closest(q))), B, B/ms*1e3))
print('pair_distances ms %.3f -> %.3e cfg/s'%((ms:=t(lambda: dev.pair_distances(q))), B/ms*1e3))
print('pair_distances+witness ms %.3f -> %.3e cfg/s'%((ms:=t(lambda: dev.pair_distances(q, witness=True))), B/ms*1e3))
print('proximity jacobian rows ms %.3f -> %.3e cfg/s'%((ms:=t(lambda: dev.proximity_jacobian(q))), B/ms*1e3))
q5 = q[:10071]
print('config 5 (10071 samples): proximity records + rows ms %.3f; mask ms %.3f'%(t(lambda: dev.proximity_jacobian(q5), 20), t(lambda: dev.validity(q5, 1e-6), 20)))
# records of chosen pairs (nbk_pair_records_items) beside the all-pairs call, config 5's M = 10 071
from numbotics_amd.planning.safe_sets import distance_and_gradient
q5n = q5.cpu().numpy()
allp = t(lambda: dev.proximity_jacobian(q5), 20)
print('subset, M=10071: all pairs (%d) records + rows ms %.3f' % (sm.n_pairs, allp))
# two body pairs (link, obstacle): the first link the obstacle's records name, and the one whose primitive pairs overlap in the
# most samples (its items reach the EPA pass: the slow lanes of the item kernel)
d5 = dev.proximity_jacobian(q5n)[0]
body = {}
for p in range(sm.n_pairs):
    subj, targ = sm.pair_members(p)
    if targ in obs and arm._has(arm.collision_pairs(), subj, targ):
        body.setdefault((subj, targ), []).append(p)
first = arm.distance_to(q5n[0], obs[0])[0].subject, obs[0]
worst = max(body, key=lambda k: (d5[:, body[k]] < 0).any(axis=1).sum())
for link, target in (first, worst):
    sel = np.asarray(arm._pair_selection(sm, target, link), dtype=np.int64)
    print('  distance_and_gradient (%s, %s: %d primitive pairs, overlapping in %d samples): device call ms %.3f; NumPy in/out ms %.3f '
          '(all-pairs composition %.3f)' % (link.name, target.name, sel.size, int((d5[:, sel] < 0).any(axis=1).sum()),
                                           t(lambda: arm._subset_records(dev, q5, sel, witness=False), 20),
                                           t(lambda: distance_and_gradient(arm, q5n, link, target), 20),
                                           t(lambda: dev.proximity_jacobian(q5n)[2][:, sel], 20)))
rng = np.random.default_rng(0)
for S in (1, 4, 16):
    pairs = rng.permutation(sm.n_pairs)[:S]
    print('  pair_proximity_jacobians %2d pairs ms %.3f' % (S, t(lambda: arm.pair_proximity_jacobians(q5, pairs), 20)))
print('  closest_proximity_jacobians ms %.3f (closest alone %.3f)' % (t(lambda: arm.closest_proximity_jacobians(q5), 20), t(lambda: dev.closest(q5), 20)))
