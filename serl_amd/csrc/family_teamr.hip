// family_teamr.hip -- REMOTE-ACTOR team kernel (round 6: the seven team wavefronts + a courier on one CU, the episode's two actor wavefronts in a
// workgroup of their own on another; rollout_team.inc SERL_TEAM_REMOTE) for one dynamics code variant: family_team.hip with these two defines.
#define SERL_ACTOR_WAVES 2          // (the LDS rows and flags of a forward pass shared by several wavefronts: rollout_team.inc)
#define SERL_TEAM_REMOTE 1
#include "family_team.hip"
